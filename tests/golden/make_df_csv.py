"""Writes tests/golden/df_csv.json: for every CSV fixture under tests/golden/data_test/csvs/ and every dialect the
tests read it with, what the restatement of tests/_csv.py gives -- stats8, the header's names, the inferred types
and the cells as a string column has them (null = an empty unquoted or missing field). Run from the repository's
root: python tests/golden/make_df_csv.py. The file pins the restatement itself: tests/test_csv_cpu.py compares a
fresh run with it, so a change of the rules shows as a diff of this fixture."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
CSVS = os.path.join(HERE, "data_test", "csvs")
OUT = os.path.join(HERE, "df_csv.json")
TAB_FILES = ("spam_ham_data_w_quote.tsv", "tabs.csv")
NO_QUOTE_TOO = ("spam_ham_data_w_quote.tsv",)


def restatement():
    """tests/_csv.py by its path: `import _csv` is the C module behind the standard library's csv."""
    spec = importlib.util.spec_from_file_location("_csv_restatement", os.path.join(os.path.dirname(HERE), "_csv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dialects(name):
    sep = "\t" if name in TAB_FILES else ","
    return [(sep, '"')] + ([(sep, None)] if name in NO_QUOTE_TOO else [])


def text(b):
    return None if b is None else b.decode("utf-8", "surrogateescape")


def build():
    C = restatement()
    cases = []
    for name in sorted(os.listdir(CSVS)):
        data = open(os.path.join(CSVS, name), "rb").read()
        for sep, quote in dialects(name):
            p = C.parse(data, ord(sep), C.NO_QUOTE if quote is None else ord(quote), True)
            cases.append({"file": name, "separator": sep, "quote": quote, "stats8": list(p.stats8), "names": [text(n) for n in p.names],
                          "types": [C.TYPE_NAMES[t] for t in C.infer(p)], "cells": [[text(c) for c in row] for row in C.cells_as_text(p)]})
    return {"comment": "tests/golden/make_df_csv.py: the restatement of tests/_csv.py over tests/golden/data_test/csvs", "cases": cases}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(build(), f, indent=1, ensure_ascii=True)
        f.write("\n")
    print(OUT)
