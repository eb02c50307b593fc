"""The JSON writer (oxh_write_json_*, oxen_amd.tabular) without a GPU: the two entries are declared, exported and bound
at ABI version 5; the argument errors come back as OXH_ERR_INVALID, in the header's order, before OXH_ERR_NODEVICE;
json_text.hpp -- the code the kernels run -- in a program of its own; the Python layer's errors and `write_df`'s arms;
and the restatement of tests/_jsonwrite.py itself against an independent implementation, Python's json module."""
import json
import math
import os
import random
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi, tabular

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_jsonwrite_call", os.path.join(HERE, "_jsonwrite_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
J = K.J
INVALID, NODEVICE = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE
FUNCTIONS = ["oxh_write_json_device", "oxh_write_json_host"]


# ---------------------------------------------------------------- the ABI
def test_the_entries_are_declared_exported_and_bound(built_lib):
    assert [s for s in _capi.header_symbols() if "oxh_write_json_" in s] == FUNCTIONS
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    assert set(FUNCTIONS) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert [len(_capi.SIGNATURES[f][1]) for f in FUNCTIONS] == [17, 16]
    header = open(_capi.HEADER).read()
    section = header[header.index("JSON text: typed Arrow columns"):]
    assert header.index("CSV text: typed Arrow columns") < header.index("JSON text: typed Arrow columns")
    assert "NOT pinned by a run of polars" in section and "only column-type enum" in section
    assert "#define OXH_JSON_LINES 0" in section and "#define OXH_JSON_ARRAY 1" in section
    assert (_capi.OXH_JSON_LINES, _capi.OXH_JSON_ARRAY) == (J.LINES, J.ARRAY) == (0, 1)
    import oxen_amd

    for name in ("JsonWriteStats", "write_jsonl", "write_jsonl_device", "write_json", "write_json_device", "write_df"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert tabular.JsonWriteStats._fields == ("bytes", "escaped_cells", "deferred", "nulls")


def past_the_argument_checks(rc):
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in _capi.lib().oxh_last_error()


@pytest.mark.parametrize("fmt", K.FORMATS, ids=["lines", "array"])
def test_argument_errors_need_no_device(built_lib, fmt):
    """The host form with a NULL context (the device form's tables are tensors on a device: tests/test_json_write.py
    runs the same list over both forms): each refusal alone, then combined with every later one."""
    call, where = K.check_refusals("host", None, fmt)
    assert past_the_argument_checks(call.run(None, where, 256))


def test_native_program(built_lib, tmp_path):
    """json_text.hpp under g++, as build.py builds it: the width and the put of all 256 bytes, length == put length
    on random spans, keys that need escaping. Then the same under -fsanitize=address,undefined (a program of its
    own; nothing is loaded into python under a sanitizer)."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.JSON_WRITE_TEST], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    exe = str(tmp_path / "json_write_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.JSON_WRITE_TEST_SRC], check=True, timeout=300)
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr


def test_python_layer_argument_errors():
    col = tabular.column
    with pytest.raises(_capi.OxenError, match="Unknown file type write_df \"x.parquet\" Some\\(\"parquet\"\\)"):
        tabular.write_df({"a": col(np.arange(3))}, "x.parquet")
    with pytest.raises(_capi.OxenError, match="Unknown file type write_df \"noext\" None"):
        tabular.write_df({"a": col(np.arange(3))}, "noext")
    for fn in (tabular.write_jsonl, tabular.write_json):
        with pytest.raises(_capi.OxenError, match="cast the column"):
            fn({"a": col(np.arange(3, dtype=np.int32))})
        with pytest.raises(_capi.OxenError, match="one row count"):
            fn({"a": col(np.arange(3)), "b": col(np.arange(4))})
        with pytest.raises(_capi.OxenError, match="unknown CSV column type"):
            fn({"a": col(np.arange(3))}, types={"a": "Int32"})


def test_write_df_reaches_the_library_for_the_json_extensions(tmp_path):
    """Without a device the new arms end in the library's own error, not in "Unknown file type"; with one they write
    the file. The csv and tsv arms behave the same way, unchanged."""
    import torch

    frame = {"a": tabular.column(np.arange(3)), "s": tabular.column(["x", 'q"', None])}
    want = {"jsonl": b'{"a":0,"s":"x"}\n{"a":1,"s":"q\\""}\n{"a":2,"s":null}\n', "ndjson": None,
            "json": b'[{"a":0,"s":"x"},{"a":1,"s":"q\\""},{"a":2,"s":null}]', "csv": b'a,s\n0,x\n1,"q"""\n2,\n', "tsv": None}
    want["ndjson"], want["tsv"] = want["jsonl"], want["csv"].replace(b",", b"\t")
    for ext, text in want.items():
        path = tmp_path / ("out." + ext)
        if torch.cuda.is_available():
            assert tabular.write_df(frame, path) == text == path.read_bytes(), ext
        else:
            with pytest.raises(_capi.OxenError) as e:
                tabular.write_df(frame, path)
            assert e.value.code == NODEVICE and "Unknown file type" not in str(e.value), ext


# ---------------------------------------------------------------- the restatement itself
def test_the_two_escape_tables_agree_on_every_ascii_byte():
    for c in range(128):
        assert J.byte_text(c) == json.dumps(chr(c), ensure_ascii=False)[1:-1].encode(), c
    assert J.byte_text(0x7F) == b"\x7f" and J.byte_text(ord("/")) == b"/"
    for c in range(128, 256):
        assert J.byte_text(c) == bytes([c])
    assert J.string_text(b"") == (b'""', False) and J.string_text(b"a\nb") == (b'"a\\nb"', True)
    assert J.string_text(b"\x01") == (b'"\\u0001"', True) and J.string_text(b"\x1f\x0b") == (b'"\\u001f\\u000b"', True)
    assert J.string_text("é/\x7f".encode()) == ("\"é/\x7f\"".encode(), False)


def known(text, *rest):
    return text, (len(text),) + rest


def test_restatement_on_known_frames():
    names, types = [b"i", b'q"'], [J.INT64, J.STRING]
    cells = [[1, None], [b"", None]]
    assert J.write(names, types, cells, J.LINES) == known(b'{"i":1,"q\\"":""}\n{"i":null,"q\\"":null}\n', 1, 0, 2)
    assert J.write(names, types, cells, J.ARRAY) == known(b'[{"i":1,"q\\"":""},{"i":null,"q\\"":null}]', 1, 0, 2)
    assert J.write([b"a"], [J.INT64], [[]], J.LINES) == (b"", (0, 0, 0, 0))
    assert J.write([b'a"'], [J.INT64], [[]], J.ARRAY) == (b"[]", (2, 0, 0, 0))
    floats = [1e15, None, 0.5, float("nan"), float("-inf"), -0.0]
    assert J.write([b"x"], [J.FLOAT64], [floats], J.ARRAY) == known(
        b'[{"x":1000000000000000.0},{"x":null},{"x":0.5},{"x":null},{"x":null},{"x":-0.0}]', 0, 1, 3)
    assert J.write([b"b", b""], [J.BOOL, J.STRING64], [[True, False], [b"\t", b"\\"]], J.LINES)[0] == b'{"b":true,"":"\\t"}\n{"b":false,"":"\\\\"}\n'


PIECES = ["a", "bc", ",", '"', "\n", " ", "é", "7", "-", "'", "\t", "\r", "\\", "/", "\x7f", "\x00", "\x01", "\x1f", "\x08", "\x0c", "€", "𝄞", "{", "}", ":"]


def random_frame(rng, nrows, ncols):
    types, cells = [], []
    for _ in range(ncols):
        t = rng.choice([J.INT64, J.FLOAT64, J.BOOL, J.STRING, J.STRING64])
        column = []
        for _ in range(nrows):
            if rng.random() < 0.15:
                column.append(None)
            elif t == J.INT64:
                column.append(rng.choice([0, -1, 1 << 62, -(1 << 63), (1 << 63) - 1, rng.randrange(-10 ** 6, 10 ** 6)]))
            elif t == J.FLOAT64:
                column.append(rng.choice([0.0, -0.0, 0.5, 1e15, 1e-7, float("inf"), float("-inf"), float("nan"), rng.random(), rng.randrange(10 ** 6) / 100,
                                          K.from_bits(rng.getrandbits(64))]))
            elif t == J.BOOL:
                column.append(rng.random() < 0.5)
            else:
                column.append("".join(rng.choice(PIECES) for _ in range(rng.randrange(0, 8))).encode("utf-8"))
        types.append(t)
        cells.append(column)
    names = ["".join(rng.choice(PIECES) for _ in range(rng.randrange(0, 4))) + str(c) for c in range(ncols)]   # distinct: json.loads keeps one of equal keys
    return [n.encode("utf-8") for n in names], types, cells


def same_cell(got, v, t):
    if v is None:
        return got is None
    if t == J.FLOAT64:
        if math.isnan(v) or math.isinf(v):
            return got is None
        return isinstance(got, float) and got == v and math.copysign(1.0, got) == math.copysign(1.0, v)
    if t == J.BOOL:
        return got is v
    if t == J.INT64:
        return isinstance(got, int) and not isinstance(got, bool) and got == v
    return got == v.decode("utf-8")


def test_restatement_against_the_json_module():
    """Random frames of valid UTF-8: every line of the JSON Lines text and the whole array text json.loads to the
    cells -- a NaN or infinity as None, floats by value and -0.0 by sign -- and every string's text equals
    json.dumps(s, ensure_ascii=False). No case holds invalid UTF-8, so nothing is skipped."""
    rng = random.Random(20261021)
    for trial in range(120):
        ncols = rng.choice([1, 2, 3, 7])
        names, types, cells = random_frame(rng, rng.randrange(0, 12), ncols)
        nrows = len(cells[0])
        lines, lstats = J.write(names, types, cells, J.LINES)
        array, astats = J.write(names, types, cells, J.ARRAY)
        assert lstats[1:] == astats[1:] and lstats[0] == len(lines) and astats[0] == len(array)
        assert b"\n" not in array and lines.count(b"\n") == nrows
        assert len(array) == len(lines) + 1 if nrows else (lines, array) == (b"", b"[]")
        rows = [json.loads(line) for line in lines.decode("utf-8").splitlines(keepends=False)] if nrows else []
        assert len(lines.split(b"\n")) == nrows + 1                         # no cell's text holds a raw newline
        assert rows == json.loads(array.decode("utf-8"))
        keys = [n.decode("utf-8") for n in names]
        for r, row in enumerate(rows):
            assert list(row) == keys
            for c, t in enumerate(types):
                assert same_cell(row[keys[c]], cells[c][r], t), (trial, r, c, row[keys[c]], cells[c][r])
        for again in json.loads(array.decode("utf-8")):
            assert list(again) == keys
        for column, t in zip(cells + [names], types + [J.STRING]):
            for v in column:
                if isinstance(v, bytes):
                    text, escaped = J.string_text(v)
                    assert text == json.dumps(v.decode("utf-8"), ensure_ascii=False).encode("utf-8")
                    assert escaped == (len(text) != len(v) + 2)
        nulls = sum(v is None or (t == J.FLOAT64 and (math.isnan(v) or math.isinf(v))) for col, t in zip(cells, types) for v in col)
        assert lstats[3] == nulls and lstats[2] == sum(J.float_deferred(v) for col, t in zip(cells, types) if t == J.FLOAT64 for v in col if v is not None)
