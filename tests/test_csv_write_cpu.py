"""The CSV writer (oxh_write_csv_*, oxen_amd.tabular) without a GPU: the two entries are declared, exported and bound
at ABI version 5; the argument errors come back as OXH_ERR_INVALID, in the header's order, before OXH_ERR_NODEVICE;
csv_text.hpp -- the code the kernels run -- in a program of its own, with the exact path against std::to_chars over
10 M and more values; and the restatement of tests/_csvwrite.py itself: against the table of edge values, through
the reader's restatement (tests/_csv.py) and back, and against Python's csv.writer."""
import csv
import ctypes
import io
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi, tabular

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_csvwrite_call", os.path.join(HERE, "_csvwrite_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
W = K.W
C = K.load("_csv_restatement", os.path.join(HERE, "_csv.py"))
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
FORMS = ["host", "device"]
FUNCTIONS = ["oxh_write_csv_device", "oxh_write_csv_host"]

# value -> text, and whether the device defers it (include/oxen_hash.h "CSV text")
EDGES = [
    (0.0, b"0.0", False), (-0.0, b"-0.0", False),
    (K.from_bits(0x7FF8000000000000), b"NaN", False), (K.from_bits(0xFFF8000000000000), b"NaN", False),
    (K.from_bits(0x7FF80000DEADBEEF), b"NaN", False), (float("inf"), b"inf", False), (float("-inf"), b"-inf", False),
    (0.1, b"0.1", False), (19.0, b"19.0", False), (1e-5, b"0.00001", False), (1e-6, b"1e-6", False), (1.5e-7, b"1.5e-7", False),
    (1.25e-7, b"1.25e-7", False), (1e-22, b"1e-22", False), (999999999999999.0, b"999999999999999.0", False),
    (1e15, b"1000000000000000.0", True), (1e16, b"1e16", True), (1.5e16, b"1.5e16", True),
    (123456789012345680.0, b"1.2345678901234568e17", True), (0.1 + 0.2, b"0.30000000000000004", True), (5e-324, b"5e-324", True),
    (2.2250738585072014e-308, b"2.2250738585072014e-308", True), (1.7976931348623157e308, b"1.7976931348623157e308", True),
    (-12.5, b"-12.5", False), (1e-23, b"1e-23", True), (1234567890123456.0, b"1234567890123456.0", True),
]


# ---------------------------------------------------------------- the ABI
def test_the_entries_are_declared_exported_and_bound(built_lib):
    assert [s for s in _capi.header_symbols() if "oxh_write_csv_" in s] == FUNCTIONS
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    assert set(FUNCTIONS) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert [len(_capi.SIGNATURES[f][1]) for f in FUNCTIONS] == [19, 18]
    header = open(_capi.HEADER).read()
    assert "CSV text" in header and "NOT pinned by a run of polars" in header
    assert (W.INT64, W.FLOAT64, W.BOOL, W.STRING, W.STRING64) == (
        _capi.OXH_CSV_INT64, _capi.OXH_CSV_FLOAT64, _capi.OXH_CSV_BOOL, _capi.OXH_CSV_STRING, _capi.OXH_CSV_STRING64)
    import oxen_amd

    for name in ("CsvWriteStats", "write_csv", "write_csv_device", "write_df"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert tabular.CsvWriteStats._fields == ("bytes", "quoted_cells", "deferred", "nulls")


def past_the_argument_checks(rc):
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in _capi.lib().oxh_last_error()


def test_argument_errors_need_no_device(built_lib):
    """The host form with a NULL context (the device form's tables are tensors on a device: tests/test_csv_write.py runs
    the same list over both forms)."""
    call, where = K.check_refusals("host", None)
    assert past_the_argument_checks(call.run(None, where, 256))


def test_native_program_exact_path_and_text(built_lib, tmp_path):
    """csv_text.hpp under g++, as build.py builds it: the integer text, the edge table, the quoting, and the exact
    path against std::to_chars -- at least 10 M values of four classes, zero mismatches; the hit rate is printed and
    is no threshold. Then a smaller run under -fsanitize=address,undefined (a program of its own; nothing is loaded
    into python under a sanitizer)."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.CSV_WRITE_TEST], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    m = re.search(r"exact path: values=(\d+) hits=(\d+) mismatches=(\d+)", r.stdout)
    assert m and int(m.group(1)) >= 10_000_000 and int(m.group(2)) > 0 and int(m.group(3)) == 0, r.stdout
    exe = str(tmp_path / "csv_write_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.CSV_WRITE_TEST_SRC], check=True, timeout=300)
    r = subprocess.run([exe, "50000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr


def test_python_layer_argument_errors():
    col = tabular.column
    with pytest.raises(_capi.OxenError, match="Unknown file type write_df \"x.parquet\" Some\\(\"parquet\"\\)"):
        tabular.write_df({"a": col(np.arange(3))}, "x.parquet")
    with pytest.raises(_capi.OxenError, match="Unknown file type write_df \"noext\" None"):
        tabular.write_df({"a": col(np.arange(3))}, "noext")
    with pytest.raises(_capi.OxenError, match="cast the column"):
        tabular.write_csv({"a": col(np.arange(3, dtype=np.int32))})
    with pytest.raises(_capi.OxenError, match="cast the column"):
        tabular.write_csv({"a": col(np.arange(3).astype("datetime64[ms]"))})
    with pytest.raises(_capi.OxenError, match="one row count"):
        tabular.write_csv({"a": col(np.arange(3)), "b": col(np.arange(4))})
    with pytest.raises(_capi.OxenError, match="one byte"):
        tabular.write_csv({"a": col(np.arange(3))}, delimiter=",,")
    with pytest.raises(_capi.OxenError, match="unknown CSV column type"):
        tabular.write_csv({"a": col(np.arange(3))}, types={"a": "Int32"})


# ---------------------------------------------------------------- the restatement itself
def test_restatement_against_the_edge_table():
    for value, text, deferred in EDGES:
        assert W.float_text(value) == text, (value, W.float_text(value), text)
        assert W.float_deferred(value) == deferred, (value, deferred)
    for v in [0, 1, -1, (1 << 63) - 1, -(1 << 63)] + [s * (10 ** k + d) for k in range(1, 19) for d in (-1, 0, 1) for s in (1, -1)]:
        assert W.cell_text(W.INT64, v, 0x2C, 0x22) == (str(v).encode(), False, False)
    assert W.cell_text(W.BOOL, True, 0x2C, 0x22)[0] == b"true" and W.cell_text(W.BOOL, False, 0x2C, 0x22)[0] == b"false"
    for raw, text in [(b"", b'""'), (b",", b'","'), (b'"', b'""""'), (b"\n", b'"\n"'), (b"\r", b'"\r"'), (b'a"b', b'"a""b"'), (b"a b", b"a b"),
                      (b'""', b'""""""'), (b"\xff\xfe", b"\xff\xfe")]:
        assert W.string_text(raw, 0x2C, 0x22) == (text, text != raw), raw
    assert W.string_text(b"a\tb", 0x09, 0x22) == (b'"a\tb"', True) and W.string_text(b"a,b", 0x09, 0x22) == (b"a,b", False)
    data, stats = W.write([b"i", b"a,b"], [W.INT64, W.STRING], [[1, None], [b"", None]])
    assert data == b'i,"a,b"\n1,""\n,\n' and stats == (len(data), 2, 0, 2)
    assert W.write([b"a"], [W.INT64], [[]]) == (b"a\n", (2, 0, 0, 0))
    assert W.write([b"a"], [W.FLOAT64], [[1e15, None, 0.5]], header=False) == (b"1000000000000000.0\n\n0.5\n", (24, 0, 1, 1))


def random_frame(rng, nrows, ncols, strings_nonempty=False, no_cr=False):
    alphabet = [b"a", b"bc", b",", b'"', b"\n", b" ", b"\xc3\xa9", b"7", b"-", b"'", b"\t"] + ([] if no_cr else [b"\r"])
    types, cells = [], []
    for _ in range(ncols):
        t = rng.choice([W.INT64, W.FLOAT64, W.BOOL, W.STRING, W.STRING64])
        column = []
        for _ in range(nrows):
            if rng.random() < 0.15:
                column.append(None)
            elif t == W.INT64:
                column.append(rng.choice([0, -1, 1 << 62, -(1 << 63), rng.randrange(-10 ** 6, 10 ** 6)]))
            elif t == W.FLOAT64:
                column.append(rng.choice([0.0, -0.0, 0.5, 1e15, 1e-7, float("inf"), float("-inf"), float("nan"), rng.random(), rng.randrange(10 ** 6) / 100,
                                          K.from_bits(rng.getrandbits(64))]))
            elif t == W.BOOL:
                column.append(rng.random() < 0.5)
            else:
                s = b"".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 6)))
                column.append(s if s or not strings_nonempty else b"x")
        types.append(t)
        cells.append(column)
    return [b"c%d" % c for c in range(ncols)], types, cells


def test_restatement_round_trip_through_the_readers_restatement():
    """The written text, read by tests/_csv.py under the written types, gives the cells back: integers, booleans and
    strings exactly (the empty string as an empty string), floats bit for bit but every NaN as the quiet NaN with its
    sign lost, nulls as nulls, the names as the names. One-column frames lose their null rows and nothing else."""
    rng = random.Random(20261020)
    for trial in range(60):
        ncols = rng.choice([1, 2, 3, 7])
        names, types, cells = random_frame(rng, rng.randrange(0, 12), ncols)
        names[0] = rng.choice([b"plain", b"a,b", b'say "hi"', b"two\nlines"])
        data, _ = W.write(names, types, cells)
        p = C.parse(data)
        assert p.names == names
        rows = list(zip(*cells)) if cells and cells[0] else []
        if ncols == 1:
            rows = [r for r in rows if r[0] is not None]        # the stated limit: an empty record is skipped
        assert p.stats8[1] == len(rows) and (p.ncols == ncols)
        for c, t in enumerate(types):
            b = C.column(p, c, t)
            valid = np.unpackbits(b.validity, bitorder="little")[:len(rows)].astype(bool)
            assert valid.tolist() == [r[c] is not None for r in rows], (trial, c)
            for r, row in enumerate(rows):
                v = row[c]
                if v is None:
                    continue
                if t == W.INT64:
                    assert int(b.values[r].astype(np.int64)) == v
                elif t == W.FLOAT64:
                    want = C.QUIET_NAN if v != v else K.to_bits(v)
                    assert int(b.values[r]) == want, (v, hex(int(b.values[r])))
                elif t == W.BOOL:
                    assert bool(np.unpackbits(b.values, bitorder="little")[r]) == v
                else:
                    assert b.values[int(b.offsets[r]):int(b.offsets[r + 1])].tobytes() == v


def test_restatement_against_the_csv_module():
    """A second, outside opinion on the quoting: Python's csv.writer with QUOTE_MINIMAL and lineterminator "\\n", on
    frames of at least two columns whose string cells are non-empty and hold no '\\r'. Narrowed classes: the standard
    library writes an empty string without quotes where the rule here writes "" (so no empty strings, and at least
    two columns, where a null row is a record of separators and not an empty line), and quotes a cell that holds
    '\\r' as the rule does but only because '\\r' is in its lineterminator set of specials -- left out as the issue
    states. Numbers and booleans go in as the restatement's own text: the csv module has no opinion on them."""
    rng = random.Random(7)
    for trial in range(80):
        ncols = rng.choice([2, 3, 5])
        names, types, cells = random_frame(rng, rng.randrange(0, 10), ncols, strings_nonempty=True, no_cr=True)
        for sep in (",", "\t"):
            data, _ = W.write(names, types, cells, sep=ord(sep))
            out = io.StringIO(newline="")
            w = csv.writer(out, delimiter=sep, quotechar='"', quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
            w.writerow([n.decode("latin-1") for n in names])
            for row in zip(*cells):
                w.writerow(["" if v is None else (v.decode("latin-1") if isinstance(v, bytes) else W.cell_text(t, v, ord(sep), 0x22)[0].decode())
                            for v, t in zip(row, types)])
            assert out.getvalue().encode("latin-1") == data, (trial, sep)
