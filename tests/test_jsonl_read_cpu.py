"""The JSON Lines reader (oxh_jsonl_*, oxen_amd.tabular) without a GPU: the seven entries are declared, exported
and bound at ABI version 5; the argument errors come back as OXH_ERR_INVALID, in the header's order, before
OXH_ERR_NODEVICE, and an empty buffer is a valid empty handle that needs no device; read_df's dispatch and its
error texts; the grammar, the unescape step, the key compare, the carries and the host pieces in a program of their
own, plain and under the sanitizers; and the restatement of tests/_jsonl.py itself against Python's json module,
pinned by tests/golden/df_jsonl.json."""
import ctypes
import importlib.util
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oxen_amd import _capi, tabular

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "data_test", "text", "test.jsonl")
GOLDEN = os.path.join(HERE, "golden", "df_jsonl.json")
FUNCTIONS = ["oxh_jsonl_close", "oxh_jsonl_columns_device", "oxh_jsonl_columns_host", "oxh_jsonl_infer", "oxh_jsonl_names",
             "oxh_jsonl_open_device", "oxh_jsonl_open_host"]
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
VP = ctypes.c_void_p
FORMS = ["host", "device"]
BS = chr(92)
U = BS + "u"


def load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


J = load("_jsonl_restatement", os.path.join(HERE, "_jsonl.py"))
make_df_jsonl = load("make_df_jsonl", os.path.join(HERE, "golden", "make_df_jsonl.py"))


# ---------------------------------------------------------------- the ABI
def test_the_entries_are_declared_exported_and_bound(built_lib):
    assert [s for s in _capi.header_symbols() if "oxh_jsonl_" in s] == FUNCTIONS
    assert not [s for s in FUNCTIONS if "oxh_csv_" in s or "oxh_write_json_" in s]
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert [len(_capi.SIGNATURES[f][1]) for f in FUNCTIONS] == [1, 11, 10, 2, 5, 8, 7]
    # the column entries take the CSV reader's parameter lists, word for word
    for form in ("device", "host"):
        assert _capi.SIGNATURES[f"oxh_jsonl_columns_{form}"] == _capi.SIGNATURES[f"oxh_csv_columns_{form}"]
    assert _capi.SIGNATURES["oxh_jsonl_names"] == _capi.SIGNATURES["oxh_csv_header"]
    header = open(_capi.HEADER).read()
    assert "JSON Lines: record index and typed Arrow columns" in header and "NOT pinned by a run of polars" in header
    assert "void* jsonl" in header and "typedef struct oxh_jsonl" not in header
    assert (J.INT64, J.FLOAT64, J.BOOL, J.STRING, J.STRING64) == (
        _capi.OXH_CSV_INT64, _capi.OXH_CSV_FLOAT64, _capi.OXH_CSV_BOOL, _capi.OXH_CSV_STRING, _capi.OXH_CSV_STRING64)
    assert J.TYPE_NAMES == tabular.CSV_TYPE_NAMES
    import oxen_amd

    for name in ("JsonlStats", "JsonlFile", "read_jsonl", "read_jsonl_device", "jsonl_shape", "jsonl_schema", "read_df"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert tabular.JsonlStats._fields == ("records", "rows", "ncols", "malformed", "skipped_blank", "non_canonical", "ignored_fields",
                                          "nested_values")
    for method in ("stats", "names", "infer", "measure", "columns", "close", "__enter__", "__exit__"):
        assert method == "stats" or hasattr(tabular.JsonlFile, method), method


def open_call(form, data=b'{"a":1}\n', nbytes=None, infer_rows=10000, flags=0, out=True, stats=True):
    L = _capi.lib()
    buf = ctypes.create_string_buffer(data, len(data)) if data is not None else None
    handle, stats8 = VP(0x1234), (ctypes.c_uint64 * 8)(*([7] * 8))
    args = [None, ctypes.cast(buf, VP) if buf is not None else None, len(data) if nbytes is None else nbytes, infer_rows, flags,
            ctypes.byref(handle) if out else None, stats8 if stats else None]
    rc = L.oxh_jsonl_open_host(*args) if form == "host" else L.oxh_jsonl_open_device(*args, None)
    return rc, handle, list(stats8)


def past_the_argument_checks(rc):
    """What a well-formed call with a NULL context gives: OXH_ERR_NODEVICE where there is no device, and the
    NULL context's own OXH_ERR_INVALID where there is one."""
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in _capi.lib().oxh_last_error()


@pytest.mark.parametrize("form", FORMS)
def test_open_argument_errors_need_no_device(built_lib, form):
    """Each is OXH_ERR_INVALID with a NULL context, in the header's order: a call with several faults names the
    first of them, and nothing is written."""
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    faults = [(dict(infer_rows=0), b"infer_rows is 0"), (dict(flags=1), b"unknown flags"), (dict(nbytes=1 << 32), b"2^32"),
              (dict(data=None, nbytes=5), b"bytes is NULL"), (dict(out=False), b"out is NULL"), (dict(stats=False), b"stats8 is NULL")]
    for k, (change, what) in enumerate(faults):
        rc, handle, stats = open_call(form, **change)
        assert rc == INVALID and what in err() and err().startswith(b"jsonl open:"), (change, err())
        assert handle.value == 0x1234 and stats == [7] * 8                       # nothing was written
        later = {}
        for more, _ in faults[k + 1:]:
            later.update(more)
        if "data" in later:
            later.pop("nbytes", None), later.update(nbytes=1 << 32)              # NULL bytes AND too many of them
        rc, _, _ = open_call(form, **{**later, **change})
        assert rc == INVALID and what in err(), (k, change, later, err())
    rc, handle, stats = open_call(form)
    assert past_the_argument_checks(rc) and handle.value == 0x1234 and stats == [7] * 8
    rc, handle, stats = open_call(form, infer_rows=(1 << 64) - 1)               # every row: no fault
    assert past_the_argument_checks(rc)


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_buffer_is_an_empty_handle_without_a_device(built_lib, form):
    L = _capi.lib()
    err = lambda: L.oxh_last_error()  # noqa: E731
    rc, handle, stats = open_call(form, data=b"")
    assert rc == OK and handle.value not in (None, 0x1234) and stats == [0] * 8
    offsets, size = (ctypes.c_uint64 * 1)(9), ctypes.c_uint64(9)
    assert L.oxh_jsonl_names(handle, None, 0, offsets, ctypes.byref(size)) == OK and size.value == 0
    assert L.oxh_jsonl_names(handle, None, 0, None, ctypes.byref(size)) == INVALID and b"name_offsets or names_bytes" in err()
    assert L.oxh_jsonl_names(None, None, 0, offsets, ctypes.byref(size)) == INVALID and b"handle" in err()
    assert L.oxh_jsonl_infer(handle, None) == OK
    assert L.oxh_jsonl_infer(None, None) == INVALID and b"handle" in err()
    columns = L.oxh_jsonl_columns_host if form == "host" else L.oxh_jsonl_columns_device
    tail = [] if form == "host" else [None]
    one, vb, st = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint64 * 1)(7), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert columns(handle, 0, None, None, None, None, None, None, None, None, *tail) == OK
    assert columns(None, 0, None, None, None, None, None, None, None, None, *tail) == INVALID and b"handle" in err()
    assert columns(handle, 1, None, one, None, None, None, None, vb, st, *tail) == INVALID and b"col_idx or types is NULL" in err()
    assert err().startswith(b"jsonl columns:")
    assert columns(handle, 1, one, one, None, None, None, None, vb, st, *tail) == INVALID and b"names column 0 of 0" in err()
    assert list(vb) == [7] and list(st) == [7] * 4
    # a CSV handle is not a JSON Lines handle, and the other way round
    assert L.oxh_csv_header(handle, None, 0, offsets, ctypes.byref(size)) == INVALID
    assert L.oxh_jsonl_close(handle) == OK and L.oxh_jsonl_close(None) == OK
    with tabular.JsonlFile(b"") as f:                                           # the Python layer over the same path
        assert f.stats == tabular.JsonlStats(*[0] * 8) and f.names == [] and f.infer() == [] and f.columns([], []) == []
    assert tabular.read_jsonl(b"") == {} and tabular.jsonl_shape(b"") == (0, 0) and tabular.jsonl_schema(b"") == []


def test_read_df_dispatch_and_its_error_texts(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(tabular, "read_csv", lambda path, ctx=None: calls.append(("csv", path)) or {})
    monkeypatch.setattr(tabular, "read_jsonl", lambda path, ctx=None: calls.append(("jsonl", path)) or {})
    for name, kind in (("a.csv", "csv"), ("b.data", "csv"), ("c.tsv", "csv"), ("d.jsonl", "jsonl"), ("e.ndjson", "jsonl")):
        assert tabular.read_df(tmp_path / name) == {} and calls[-1] == (kind, str(tmp_path / name))
    for ext in ("json", "parquet", "arrow"):
        with pytest.raises(_capi.OxenError, match=f'reading the "{ext}" form is not built'):
            tabular.read_df(f"x.{ext}")
    with pytest.raises(_capi.OxenError) as e:
        tabular.read_df("dir/x.txt")
    assert 'Could not load data frame with path: "dir/x.txt" and extension: txt' in str(e.value)
    with pytest.raises(_capi.OxenError) as e:
        tabular.read_df("noext")
    assert 'Could not load data frame with path: "noext" and extension: None' in str(e.value)
    assert len(calls) == 5
    assert tabular._READ_ERROR == "Could not read tabular data from path"


def test_grammar_carries_and_host_pieces_native_program(built_lib, tmp_path):
    """jsonl_text.hpp -- the code the kernels run --, its carries folded as the kernels fold them against a
    byte-by-byte walk, and jsonl_host.hpp in a program of their own: as build.py builds it, and under
    -fsanitize=address,undefined. Nothing is loaded into python under a sanitizer."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.JSONL_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    exe = str(tmp_path / "jsonl_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.JSONL_TEST_SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---------------------------------------------------------------- the restatement against Python's json
def strict_loads(text):
    def refuse(name):
        raise ValueError(name)

    return json.loads(text, parse_constant=refuse)


STRINGS = ["", "plain", "with space", "tr" + chr(0xE9) + "s", chr(0x20AC) + " euro", chr(0x1F600) + " face", "q\"uote", "back" + BS + "slash",
           "a/b", "\b\f\n\r\t", chr(0) + "nul", chr(0x7F), "{not: [structure]}", 'x",":1,"y', BS + BS + '"', "x" * 70]
NUMBERS = ["0", "-0", "7", "-12", "9223372036854775807", "-9223372036854775808", "9223372036854775808", "12345678901234567890", "1.5", "-0.0",
           "1e3", "1E-3", "2.5e+10", "1e400", "-1e400", "1e-400", "0.1", "123456789.123456789", "9007199254740993", "1.7976931348623157e308", "5e-324",
           "0.30000000000000004", "1" + "0" * 25, "0." + "0" * 25 + "1"]
NESTED = ["[]", "{}", "[1, 2.5, \"x\"]", "{\"k\": [1, {\"d\": \"}]\"}], \"s\": \"a,b:c\"}", "[[[]]]", "[\"" + BS + "\"\", \"]\"]"]
KEYS = ["a", "b c", "k" + chr(0xE9), "d\"q", "e" + BS + "e", "f", "g"]


def escape_string(rng, s: str) -> str:
    """s as a JSON string token, each character in one of its spellings."""
    out = ['"']
    short = {'"': BS + '"', BS: BS + BS, "/": BS + "/", "\b": BS + "b", "\f": BS + "f", "\n": BS + "n", "\r": BS + "r", "\t": BS + "t"}
    for ch in s:
        cp, pick = ord(ch), rng.integers(4)
        if cp >= 0x10000 and pick < 2:
            hi, lo = 0xD800 + ((cp - 0x10000) >> 10), 0xDC00 + ((cp - 0x10000) & 0x3FF)
            out.append(f"{U}{hi:04x}{U}{lo:04X}")
        elif ch in short and (pick < 3 or ch in ('"', BS) or cp < 0x20):
            out.append(short[ch] if pick or cp >= 0x20 else f"{U}{cp:04x}")
        elif cp < 0x20 or (pick == 0 and cp < 0x10000):
            out.append(f"{U}{cp:04X}" if pick % 2 else f"{U}{cp:04x}")
        else:
            out.append(ch)
    return "".join(out) + '"'


def generated_lines(seed=5, count=400):
    rng = np.random.default_rng(seed)
    ws = lambda: "".join(rng.choice([" ", "\t", "\r", ""], size=rng.integers(3)))   # noqa: E731
    lines = []
    for _ in range(count):
        keys = [KEYS[k] for k in rng.permutation(len(KEYS))[:rng.integers(len(KEYS) + 1)]]
        fields = []
        for key in keys:
            what = rng.integers(6)
            value = (escape_string(rng, STRINGS[rng.integers(len(STRINGS))]) if what == 0 else NUMBERS[rng.integers(len(NUMBERS))] if what in (1, 2)
                     else NESTED[rng.integers(len(NESTED))] if what == 3 else ["true", "false", "null"][rng.integers(3)])
            fields.append(f"{ws()}{escape_string(rng, key)}{ws()}:{ws()}{value}{ws()}")
        lines.append(f"{ws()}{{{','.join(fields) if fields else ws()}}}{ws()}")
    return lines


def check_cell(slot: bytes, want):
    """One trimmed value slot against what json.loads made of the same text."""
    kind = J.kind_of(slot)
    assert kind != J.UNPARSABLE, slot
    if want is None:
        assert kind == J.NULL
    elif isinstance(want, bool):
        assert kind == (J.TRUE if want else J.FALSE) and J.cell_value(slot, J.BOOL) == ("ok", want)
    elif isinstance(want, str):
        assert kind == J.STR and J.cell_value(slot, J.STRING) == ("ok", want.encode("utf-8", errors="surrogatepass")), slot
    elif isinstance(want, int):
        assert kind == J.INTEGER
        if -(1 << 63) <= want < 1 << 63:
            assert J.cell_value(slot, J.INT64) == ("ok", want)
        else:
            assert J.cell_value(slot, J.INT64) == ("bad",)
        assert J.cell_value(slot, J.FLOAT64)[1] == struct.unpack("<Q", struct.pack("<d", float(slot)))[0]
    elif isinstance(want, float):
        assert kind == J.NUMBER and J.cell_value(slot, J.INT64) == ("bad",)
        assert J.cell_value(slot, J.FLOAT64)[1] == struct.unpack("<Q", struct.pack("<d", float(slot)))[0]
        assert struct.pack("<d", want) == struct.pack("<d", float(slot))
    else:
        assert kind == J.NESTED and strict_loads(J.cell_value(slot, J.STRING)[1].decode("utf-8")) == want


def test_restatement_against_json_on_generated_lines():
    lines = generated_lines()
    text = "\n".join(lines)
    for needle in (U + "d8", BS + "n", BS + "/", "1e400", "-0", "12345678901234567890", chr(0xE9), "\t", "\r", "[[[]]]", "{}"):
        assert needle in text, needle
    data = text.encode("utf-8")
    p = J.parse(data, infer_rows=1 << 62)
    assert p.stats8[0] == len(lines) and p.stats8[3] == p.stats8[4] == p.stats8[6] == 0      # no line malformed, blank or ignored
    assert sorted(p.names) == sorted(k.encode("utf-8") for k in KEYS)
    seen = set()
    for line, row in zip(lines, p.rows):
        want = strict_loads(line)
        assert {p.names[c].decode("utf-8") for c in range(p.ncols) if row[c] is not None} == set(want)
        for c in range(p.ncols):
            if row[c] is not None:
                check_cell(row[c], want[p.names[c].decode("utf-8")])
                seen.add(J.kind_of(row[c]))
    assert seen == {J.STR, J.NESTED, J.TRUE, J.FALSE, J.NULL, J.INTEGER, J.NUMBER}
    # the keys of each line in the order written: canonical exactly when they are a prefix of the names
    canonical = sum(list(strict_loads(line)) == [n.decode("utf-8") for n in p.names[:len(strict_loads(line))]] for line in lines)
    assert p.stats8[5] == len(lines) - canonical and 0 < canonical < len(lines)


MALFORMED = ['{"a":1,}', '{"a" 1}', '{"a":01}', '{"a":1.}', '{"a":.5}', '{"a":tru}', '{"a":"x\ty"}', '{"a":"' + BS + 'x"}', '{"a":"x' + BS + '"}',
             '{"a":"x}', '{"a":1} {"b":2}', '{"a":1} x', '{"a":}', '{:1}', '{"a":1]', '{a:1}', "{'a':1}", '{"a":1 "b":2}',
             '{"a":+1}', '{"a":NaN}', '{"a":Infinity}', '{"a":True}', '{"a":"' + U + '12"}', '{"a":[1,2}', '{"a":"x" "y"}']


@pytest.mark.parametrize("line", MALFORMED)
def test_malformed_lines_are_flagged_and_stay_on_their_line(line):
    with pytest.raises(ValueError):
        strict_loads(line)
    data = ('{"a":5}\n' + line + '\n{"a":6, "b":"after"}\n').encode("utf-8")
    p = J.parse(data)
    assert p.stats8[0] == 3
    bad_record = p.stats8[3] == 1
    a = J.column(p, 0, J.STRING)
    assert bad_record or a.stats4[1] == 1, line                                   # a malformed record or an unparsable cell
    if bad_record:
        assert p.rows[1] == [None] * p.ncols
    # the lines around it are whole
    assert p.rows[0][0] == b"5" and p.rows[2][0] == b"6" and p.rows[2][p.names.index(b"b")] == b'"after"'


def test_a_line_that_is_json_but_no_object_is_a_malformed_record():
    for line in ("[1]", '"s"', "12", "null", '[{"a":1}]'):
        strict_loads(line)
        p = J.parse(('{"a":5}\n' + line + "\n").encode())
        assert p.stats8[:4] == (2, 2, 1, 1) and p.rows == [[b"5"], [None]], line


def test_the_two_deliberate_differences_from_python():
    # a lone surrogate: Python makes a str that is no UTF-8; here the token is unparsable
    for tok in ('"' + U + 'd83d"', '"' + U + 'de00 x"', '"' + U + 'd83d' + BS + 'n"', '"' + U + 'd83d' + U + 'd83d"'):
        assert isinstance(strict_loads(tok), str) and J.string_value(tok.encode()) is None and J.kind_of(tok.encode()) == J.UNPARSABLE
    # a repeated key: Python keeps the last, here the first wins
    line = '{"a": 1, "b": 2, "a": 3}'
    assert strict_loads(line) == {"a": 3, "b": 2}
    p = J.parse(line.encode())
    assert p.names == [b"a", b"b"] and p.rows == [[b"1", b"2"]] and p.stats8[5] == 1 and p.stats8[6] == 0


def test_names_window_and_counts_of_the_restatement():
    data = ('{"a":1}\n{"b":2,"a' + U + '0062":3}\n\n{"a":4,"c":{"x":1},"ab":5}\n \t\r\n{"c":6}').encode()
    p = J.parse(data, infer_rows=2)
    assert p.names == [b"a", b"b", b"ab"] and p.stats8 == (4, 4, 3, 0, 2, 3, 2, 1) and p.window == 2
    assert p.rows == [[b"1", None, None], [None, b"2", b"3"], [b"4", None, b"5"], [None, None, None]]
    assert J.infer(p) == [J.INT64, J.INT64, J.INT64]
    q = J.parse(data, infer_rows=10000)
    assert q.names == [b"a", b"b", b"ab", b"c"] and q.stats8[5:] == (3, 0, 1) and J.infer(q)[3] == J.STRING
    assert J.lines_of(b"") == [] and J.lines_of(b"\n\n") == [(0, 0), (1, 1)] and J.lines_of(b"a\nb") == [(0, 1), (2, 3)]
    assert J.parse(b"\n \n\r\n").stats8 == (0, 0, 0, 0, 3, 0, 0, 0)
    assert J.parse(b"\xef\xbb\xbf{\"a\":1}\n").stats8[3] == 1                  # a BOM is not skipped


def test_golden_fixture_is_what_the_restatement_gives():
    want = json.load(open(GOLDEN))
    assert make_df_jsonl.build() == want
    by = {c["name"]: c for c in want["cases"]}
    fixture = by["test.jsonl"]
    assert fixture["names"] == ["id", "text", "category"] and fixture["types"] == ["Int64", "String", "String"]
    assert fixture["stats8"] == [2, 2, 3, 0, 0, 0, 0, 0]
    assert fixture["cells"] == [["1", "I love it", "positive"], ["1", "I hate it", "negative"]]
    assert [json.loads(line) for line in open(FIXTURE)] == [dict(zip(fixture["names"], [int(r[0]), r[1], r[2]])) for r in fixture["cells"]]
    assert by["rules"]["stats8"][3:5] == [5, 2] and by["rules, a window of 2"]["stats8"][6] == 2
