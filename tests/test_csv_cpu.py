"""The CSV reader (oxh_csv_*, oxen_amd.tabular) without a GPU: the seven entries are declared, exported and bound
at ABI version 5; the argument errors come back as OXH_ERR_INVALID, in the header's order, before
OXH_ERR_NODEVICE, and an empty buffer is a valid empty handle that needs no device; the parsers (csv_number.hpp,
the code the kernels run) and the host pieces in a program of their own, plain and under the sanitizers; and the
restatement of tests/_csv.py itself against Python's csv module and, where it imports, pyarrow.csv, and pinned by
tests/golden/df_csv.json."""
import csv
import ctypes
import importlib.util
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oxen_amd import _capi, tabular

HERE = os.path.dirname(os.path.abspath(__file__))
CSVS = os.path.join(HERE, "golden", "data_test", "csvs")
GOLDEN = os.path.join(HERE, "golden", "df_csv.json")
FUNCTIONS = ["oxh_csv_close", "oxh_csv_columns_device", "oxh_csv_columns_host", "oxh_csv_header", "oxh_csv_infer",
             "oxh_csv_open_device", "oxh_csv_open_host"]
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
VP = ctypes.c_void_p
FORMS = ["host", "device"]


def load(name, path):
    """A module by its path: `import _csv` is the C module behind the standard library's csv."""
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


C = load("_csv_restatement", os.path.join(HERE, "_csv.py"))
make_df_csv = load("make_df_csv", os.path.join(HERE, "golden", "make_df_csv.py"))


# ---------------------------------------------------------------- the ABI
def test_the_entries_are_declared_exported_and_bound(built_lib):
    assert [s for s in _capi.header_symbols() if "oxh_csv_" in s] == FUNCTIONS
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert [len(_capi.SIGNATURES[f][1]) for f in FUNCTIONS] == [1, 11, 10, 5, 3, 9, 8]
    header = open(_capi.HEADER).read()
    for name in ("OXH_CSV_NO_QUOTE", "OXH_CSV_HAS_HEADER", "OXH_CSV_INT64", "OXH_CSV_FLOAT64", "OXH_CSV_BOOL", "OXH_CSV_STRING",
                 "OXH_CSV_STRING64"):
        assert f"#define {name} {getattr(_capi, name)}\n" in header, name
    assert (C.NO_QUOTE, C.INT64, C.FLOAT64, C.BOOL, C.STRING, C.STRING64) == (
        _capi.OXH_CSV_NO_QUOTE, _capi.OXH_CSV_INT64, _capi.OXH_CSV_FLOAT64, _capi.OXH_CSV_BOOL, _capi.OXH_CSV_STRING, _capi.OXH_CSV_STRING64)
    assert C.TYPE_NAMES == tabular.CSV_TYPE_NAMES
    assert "NOT pinned by\n * a run of polars" in header and "void* csv" in header and "typedef struct oxh_csv" not in header
    import oxen_amd

    for name in ("CsvStats", "CsvColumnStats", "CsvFile", "CSV_TYPE_NAMES", "read_csv", "read_csv_device", "csv_shape", "csv_schema"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert tabular.CsvStats._fields == ("records", "rows", "ncols", "delimiters", "skipped_empty", "short_records", "long_records",
                                        "ended_in_quotes")
    assert tabular.CsvColumnStats._fields == ("null_empty", "null_unparsable", "deferred", "value_bytes")


def open_call(form, data=b"a,b\n", nbytes=None, sep=0x2C, quote=0x22, flags=1, out=True, stats=True):
    L = _capi.lib()
    buf = ctypes.create_string_buffer(data, len(data)) if data is not None else None
    handle, stats8 = VP(0x1234), (ctypes.c_uint64 * 8)(*([7] * 8))
    args = [None, ctypes.cast(buf, VP) if buf is not None else None, len(data) if nbytes is None else nbytes, sep, quote, flags,
            ctypes.byref(handle) if out else None, stats8 if stats else None]
    rc = L.oxh_csv_open_host(*args) if form == "host" else L.oxh_csv_open_device(*args, None)
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
    first of them."""
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    faults = [(dict(sep=256), b"separator is not one byte"), (dict(quote=257), b"quote is neither"), (dict(sep=0x0A), b"separator is a line end"),
              (dict(quote=0x0D), b"quote is a line end"), (dict(quote=0x2C), b"quote is the separator"), (dict(flags=2), b"unknown flags"),
              (dict(nbytes=1 << 32), b"2^32"), (dict(data=None, nbytes=5), b"bytes is NULL"), (dict(out=False), b"out is NULL"),
              (dict(stats=False), b"stats8 is NULL")]
    for k, (change, what) in enumerate(faults):
        rc, handle, stats = open_call(form, **change)
        assert rc == INVALID and what in err() and b"csv open" in err(), (change, err())
        assert handle.value == 0x1234 and stats == [7] * 8                       # nothing was written
        later = {}
        for more, _ in faults[k + 1:]:
            later.update(more)
        if "data" in later:
            later.pop("nbytes", None), later.update(nbytes=1 << 32)              # NULL bytes AND too many of them
        if change.get("sep") == 0x0A:
            later.pop("quote", None)
        rc, _, _ = open_call(form, **{**later, **change})
        assert rc == INVALID and what in err(), (k, change, later, err())
    rc, handle, stats = open_call(form)
    assert past_the_argument_checks(rc) and handle.value == 0x1234 and stats == [7] * 8


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_buffer_is_an_empty_handle_without_a_device(built_lib, form):
    L = _capi.lib()
    err = lambda: L.oxh_last_error()  # noqa: E731
    rc, handle, stats = open_call(form, data=b"", quote=_capi.OXH_CSV_NO_QUOTE)
    assert rc == OK and handle.value not in (None, 0x1234) and stats == [0] * 8
    offsets, size = (ctypes.c_uint64 * 1)(9), ctypes.c_uint64(9)
    assert L.oxh_csv_header(handle, None, 0, offsets, ctypes.byref(size)) == OK and size.value == 0
    assert L.oxh_csv_header(handle, None, 0, None, ctypes.byref(size)) == INVALID and b"name_offsets or names_bytes" in err()
    assert L.oxh_csv_header(None, None, 0, offsets, ctypes.byref(size)) == INVALID and b"handle" in err()
    assert L.oxh_csv_infer(handle, 100, None) == OK
    assert L.oxh_csv_infer(None, 100, None) == INVALID and b"handle" in err()
    columns = L.oxh_csv_columns_host if form == "host" else L.oxh_csv_columns_device
    tail = [] if form == "host" else [None]
    one, vb, st = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint64 * 1)(7), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert columns(handle, 0, None, None, None, None, None, None, None, None, *tail) == OK
    assert columns(None, 0, None, None, None, None, None, None, None, None, *tail) == INVALID and b"handle" in err()
    assert columns(handle, 1, None, one, None, None, None, None, vb, st, *tail) == INVALID and b"col_idx or types is NULL" in err()
    assert columns(handle, 1, one, one, None, None, None, None, vb, st, *tail) == INVALID and b"names column 0 of 0" in err()
    assert list(vb) == [7] and list(st) == [7] * 4
    assert L.oxh_csv_close(handle) == OK and L.oxh_csv_close(None) == OK


def test_parsers_and_host_pieces_native_program(built_lib, tmp_path):
    """csv_number.hpp -- the code the kernels run --, the argument checks (those of oxh_csv_columns_* included), the
    refusal of an OXH_CSV_STRING column at 2^31 bytes, the leases and the deferred conversion in a program of their
    own: as build.py builds it, and under -fsanitize=address,undefined. Nothing is loaded into python under a
    sanitizer."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.CSV_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    exe = str(tmp_path / "csv_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.CSV_TEST_SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_python_layer_argument_errors():
    with pytest.raises(_capi.OxenError, match="one byte"):
        tabular.CsvFile(b"a\n", delimiter="ab")
    with pytest.raises(_capi.OxenError, match="one byte"):
        tabular.CsvFile(b"a\n", quote_char="")
    assert tabular._csv_delimiter(None, "x/Data.TSV") == "\t" and tabular._csv_delimiter(None, "x.csv") == "," == tabular._csv_delimiter(None, None)
    assert tabular._csv_delimiter(";", "x.tsv") == ";"
    assert tabular._csv_type("Float64") == _capi.OXH_CSV_FLOAT64 and tabular._csv_type(5) == 5
    with pytest.raises(_capi.OxenError, match="unknown CSV column type"):
        tabular._csv_type("Date")


# ---------------------------------------------------------------- the restatement
def csv_module_rows(data: bytes, sep: str, quote):
    text = data.decode("latin-1")   # one character per byte
    kw = dict(delimiter=sep, quotechar=quote, doublequote=True) if quote else dict(delimiter=sep, quoting=csv.QUOTE_NONE)
    return [[cell.encode("latin-1") for cell in row] for row in csv.reader(io.StringIO(text, newline=""), **kw) if row]


def restated_records(data: bytes, sep: str, quote):
    """Every kept record's field values, before the ragged rule."""
    q = C.NO_QUOTE if quote is None else ord(quote)
    records, _ = C.tokenize(data, ord(sep), q)
    out = []
    for fields in records:
        raws = [data[a:b] for a, b in fields]
        if raws[-1].endswith(b"\r"):
            raws[-1] = raws[-1][:-1]
        if raws != [b""]:
            out.append([C.field_value(r, q)[0] for r in raws])
    return out


def generated_files():
    rng = np.random.default_rng(11)
    pieces = [b"plain", b"", b"with space", b"1.5", b"-7", b"true", b"a,b", b"line\nbreak", b'say ""hi""', b'""', b",\n,", b"x" * 70,
              b"tr\xc3\xa9s", b"\r\nboth"]
    files = []
    for eol in (b"\n", b"\r\n"):
        for trailing in (True, False):
            lines = [b"c0,c1,c2,c3"]
            for _ in range(60):
                cells = []
                for _ in range(4):
                    v = pieces[int(rng.integers(len(pieces)))]
                    needs = any(ch in v for ch in (b",", b"\n", b'"', b"\r")) or rng.random() < 0.2
                    cells.append(b'"' + v + b'"' if needs else v)
                if cells == [b""] * 4:
                    cells[0] = b"x"
                lines.append(b",".join(cells))
            files.append(eol.join(lines) + (eol if trailing else b""))
    return files


@pytest.mark.parametrize("name", sorted(os.listdir(CSVS)))
def test_restatement_against_the_csv_module_on_the_fixtures(name):
    data = open(os.path.join(CSVS, name), "rb").read()
    sep = "\t" if name in make_df_csv.TAB_FILES else ","
    if name == "spam_ham_data_w_quote.tsv":
        # 9 quote bytes, some inside unquoted fields: the parity rule pairs them across lines (100 records), Python's
        # csv treats a quote inside an unquoted field as text (101). Without a quote byte the two agree
        assert data.count(b'"') == 9
        assert len(restated_records(data, sep, '"')) == 100 and len(csv_module_rows(data, sep, '"')) == 101
        assert len(restated_records(data, sep, None)) == 101
        assert restated_records(data, sep, None) == csv_module_rows(data, sep, None)
        return
    assert restated_records(data, sep, '"') == csv_module_rows(data, sep, '"')


def test_restatement_against_the_csv_module_on_generated_files():
    for data in generated_files():
        assert b'"' in data and b"\n" in data
        got = restated_records(data, ",", '"')
        assert got == csv_module_rows(data, ",", '"')
        p = C.parse(data)
        assert p.ncols == 4 and p.stats8[5] == p.stats8[6] == 0 and [[c[0] for c in row] for row in p.rows] == got[1:]


def test_restatement_against_pyarrow_on_generated_files():
    """The cells of well-formed files as string columns. The one known difference: pyarrow gives "" for an empty
    unquoted field of a string column, this project a null."""
    pa = pytest.importorskip("pyarrow")
    pacsv = pytest.importorskip("pyarrow.csv")
    for data in generated_files():
        table = pacsv.read_csv(io.BytesIO(data), parse_options=pacsv.ParseOptions(newlines_in_values=True),
                               convert_options=pacsv.ConvertOptions(column_types={f"c{k}": pa.string() for k in range(4)},
                                                                    strings_can_be_null=False))
        theirs = [[None if v is None else v.encode() for v in table.column(k).to_pylist()] for k in range(4)]
        ours = C.cells_as_text(C.parse(data))
        assert len(ours) == table.num_rows
        for k in range(4):
            assert [b"" if row[k] is None else row[k] for row in ours] == theirs[k], k


def test_typed_parsers_of_the_restatement():
    assert C.parse_int(b"-9223372036854775808") == -(1 << 63) and C.parse_int(b"9223372036854775808") == "range"
    assert C.parse_int(b"+") is None and C.parse_int(b"1 ") is None and C.parse_int(b"") is None
    assert C.parse_float(b"1e") is None and C.parse_float(b".") is None and C.parse_float(b"1.5\n") is None
    assert C.parse_float(b"-NaN") == (C.QUIET_NAN | 1 << 63, False) and C.parse_float(b"Infinity")[0] == 0x7FF0000000000000
    assert C.parse_float(b"9007199254740992") == (C.float_bits(2.0 ** 53), False) and C.parse_float(b"9007199254740993")[1]
    assert not C.parse_float(b"1e22")[1] and C.parse_float(b"1e23")[1] and not C.parse_float(b"0e999")[1]
    assert C.parse_float(b"1" + b"0" * 21)[1] and not C.parse_float(b"0" * 30 + b"1.5")[1]
    assert C.class_bits(b"") == 7 and C.class_bits(b"12") == 3 and C.class_bits(b"TRUE") == 4 and C.class_bits(b"x") == 0
    p = C.parse(b'a,b,c\n1,"",x\n,"",\n2.5,"",true\n')
    assert C.infer(p) == [C.FLOAT64, C.STRING, C.STRING] and C.infer(p, 1) == [C.INT64, C.STRING, C.STRING]
    b = C.column(p, 1, C.STRING)
    assert b.validity.tolist() == [0b111] and b.offsets.tolist() == [0, 0, 0, 0] and b.stats4 == (0, 0, 0, 0)    # "" is an empty string
    assert C.column(p, 1, C.INT64).stats4 == (3, 0, 0, 24) and C.column(p, 2, C.BOOL).stats4 == (1, 1, 0, 1)
    assert C.column(p, 0, C.FLOAT64).values.view(np.float64).tolist() == [1.0, 0.0, 2.5]


def test_golden_fixture_is_what_the_restatement_gives():
    want = json.load(open(GOLDEN))
    assert make_df_csv.build() == want
    by = {(c["file"], c["quote"]): c for c in want["cases"]}
    assert by[("spam_ham_data_w_quote.tsv", '"')]["stats8"][0] == 100 and by[("spam_ham_data_w_quote.tsv", None)]["stats8"][0] == 101
    assert len(want["cases"]) == len(os.listdir(CSVS)) + 1
    mixed = by[("mixed_data_types.csv", '"')]
    assert mixed["types"] == ["String", "String", "Boolean", "Float64", "Int64"] and mixed["stats8"][:3] == [len(mixed["cells"]) + 1, len(mixed["cells"]), 5]
    assert by[("empty_rows_carriage_return.csv", '"')]["stats8"] == [1, 0, 4, 4, 0, 0, 0, 0]
