"""Writes tests/golden/df_jsonl.json: what the restatement of tests/_jsonl.py makes of the JSON Lines fixture of
the data-test tree and of a few lines that meet every rule of include/oxen_hash.h "JSON Lines" once -- stats8, the
names, the inferred types and every cell as text. The file pins the restatement: a change to tests/_jsonl.py that
changes an answer shows in the diff of the JSON.

    python tests/golden/make_df_jsonl.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "data_test", "text", "test.jsonl")
OUT = os.path.join(HERE, "df_jsonl.json")
BS = chr(92)


def restatement():
    name = "_jsonl_restatement"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(HERE), "_jsonl.py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


def rules_text() -> bytes:
    """One buffer that meets each rule: escapes and a surrogate pair, an escaped key equal to a plain name, a
    repeated key, a nested value, reordered and missing keys, a key past the window's names, numbers across the
    grammar, blank lines, CRLF, malformed lines of every sort, a last line without a newline."""
    u = BS + "u"
    lines = [
        '{"id": 1, "text": "plain", "score": 1.5, "ok": true}',
        '{"id": -0, "text": "tab' + BS + 't quote' + BS + '" slash' + BS + '/ ' + u + '00e9' + u + 'd83d' + u + 'de00", "score": 1e400, "ok": false}\r',
        '',
        '  \t\r',
        '{"text": "reordered", "id": 12345678901234567890, "t' + u + '0065xt": "the first wins", "extra": [1, {"a": "}"}]}',
        '{"id": 2, "score": null, "meta": {"k": [1.0, 2.5e-3]}, "ok": "yes"}',
        '{"id": 3,}',
        '{"id" 4}',
        '{"id": 01, "text": "raw' + "\t" + 'tab", "score": .5, "ok": tru}',
        '{"id": 5} trailing',
        '{"id": 6, "text": "unclosed}',
        '{"id": 7}{"id": 8}',
        '{}',
        '{"id": 9, "text": "lone ' + u + 'd83d", "score": -1E+2}',
        '{"id": 10, "text": "last line, no newline"}',
    ]
    return "\n".join(lines).encode("utf-8")


def case(J, name: str, data: bytes, infer_rows: int) -> dict:
    p = J.parse(data, infer_rows)
    cells = []
    for r in range(len(p.rows)):
        row = []
        for c in range(p.ncols):
            got = J.cell_value(p.rows[r][c], J.STRING)
            row.append(got[1].decode("utf-8", errors="replace") if got[0] == "ok" else got[0])
        cells.append(row)
    return {"name": name, "infer_rows": infer_rows, "stats8": list(p.stats8), "names": [n.decode("utf-8") for n in p.names],
            "types": [J.TYPE_NAMES[t] for t in J.infer(p)], "cells": cells}


def build() -> dict:
    J = restatement()
    fixture = open(FIXTURE, "rb").read()
    return {"cases": [case(J, "test.jsonl", fixture, 10000), case(J, "rules", rules_text(), 10000), case(J, "rules, a window of 2", rules_text(), 2)]}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(build(), f, indent=1, sort_keys=True)
        f.write("\n")
