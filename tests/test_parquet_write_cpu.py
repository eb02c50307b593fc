"""The Parquet writer (oxh_write_parquet_*) without a GPU: the argument errors in the header's order, before
OXH_ERR_NODEVICE; parquet_host.hpp in a program of its own; the reader tests/_parquet.py pinned on files pyarrow wrote."""
import ctypes
import io
import subprocess

import numpy as np
import pytest

import _csvwrite_call as C
import _parquet as P
from oxen_amd import _capi, tabular



def test_argument_errors_need_no_device(built_lib):
    """Host form, NULL context: each refusal with every later one names the first and writes no output."""
    cols, types, _ = C.refusal_frame()
    tables = tabular._tables(cols, lambda a: None if a is None else a.ctypes.data)   # contiguous arrays that `cols` keeps alive
    n, u32s = len(cols), lambda *v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    offsets, names = np.arange(n + 1, dtype=np.uint64), np.frombuffer(b"ifbsS\0", dtype=np.uint8)
    size, stats = ctypes.c_uint64(77), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    good = dict(ctx=None, nrows=3, ncols=n, types=u32s(*types), kinds=tables[0], values=tables[1], offsets=tables[2], validity=tables[3],
                bits=tables[4], names=names.ctypes.data, name_offsets=offsets.ctypes.data_as(_capi._u64p), rows_per_group=0, page_bytes=0,
                flags=0, out=None, capacity=0, out_bytes=ctypes.byref(size), stats4=stats)
    down = np.array([0, 1, 2, 1, 4, 5], dtype=np.uint64)
    faults = [(dict(types=None), b"is NULL"), (dict(bits=None), b"is NULL"), (dict(ncols=0), b"ncols is 0"), (dict(flags=1), b"unknown flags"),
              (dict(rows_per_group=1000), b"multiple of 1024"), (dict(types=u32s(1, 2, 9, 4, 5)), b"unknown type 9"),
              (dict(kinds=u32s(4, *list(tables[0])[1:])), b"column 0 of type 1 has kind 4"), (dict(name_offsets=None), b"name_offsets is NULL"),
              (dict(name_offsets=down.ctypes.data_as(_capi._u64p)), b"name_offsets decrease"), (dict(names=None), b"names is NULL"),
              (dict(stats4=None), b"out_bytes or stats4"), (dict(nrows=(1 << 40) + 1), b"2^40"),
              (dict(values=(ctypes.c_void_p * n)(None, *list(tables[1])[1:])), b"column 0 has no values")]
    fn, err = _capi.lib().oxh_write_parquet_host, _capi.lib().oxh_last_error
    for k, (change, what) in enumerate(faults):
        later = {}
        for more, _ in reversed(faults[k + 1:]):
            later.update(more)
        assert fn(*{**good, **later, **change}.values()) == _capi.OXH_ERR_INVALID and what in err() and err().startswith(b"parquet write:"), (k, err())
        assert size.value == 77 and list(stats) == [7] * 4, "a refused call wrote an output"
    assert fn(*good.values()) == _capi.OXH_ERR_NODEVICE or b"ctx is NULL" in err()   # past the argument checks


def test_native_program(built_lib, tmp_path):
    """parquet_host.hpp as build.py builds it and under ASan / UBSan (a program of its own); its empty file reads."""
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip().endswith("ok") for r in outs) and outs[0].stdout == outs[1].stdout, [r.stderr for r in outs]
    none = P.read(b"PAR1" + bytes.fromhex(outs[0].stdout.split()[1]))
    assert none.num_rows == 0 and none.names == [b"id", b"flag", b"text"] and none.types == [P.INT64, P.BOOLEAN, P.BYTE_ARRAY] and none.groups == []


def test_the_reader_reads_what_pyarrow_wrote():
    """The reader on pyarrow's files (compression none, no dictionary, V1 pages): nulls, an all-null column, NaN, -0.0."""
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    n = 3000
    cells = {"i": [None if r % 11 == 3 else r * 7919 - (1 << 40) for r in range(n)], "b": [r % 3 == 0 for r in range(n)],
             "f": [None if r % 7 == 0 else [0.5, -0.0, float("nan"), float("inf")][r % 4] for r in range(n)],
             "nb": [None if r % 5 else r % 2 == 0 for r in range(n)], "s": [None if r % 13 == 0 else "é" * (r % 19) for r in range(n)], "z": [None] * n}
    kinds = {"i": pa.int64(), "b": pa.bool_(), "f": pa.float64(), "nb": pa.bool_(), "s": pa.string(), "z": pa.int64()}
    sink = io.BytesIO()
    pq.write_table(pa.table({k: pa.array(v, kinds[k]) for k, v in cells.items()}), sink, compression="none", use_dictionary=False,
                   data_page_version="1.0", row_group_size=1100, data_page_size=2000)
    f = P.read(sink.getvalue())
    assert f.names == [k.encode() for k in cells] and f.types == [P.INT64, P.BOOLEAN, P.DOUBLE, P.BOOLEAN, P.BYTE_ARRAY, P.INT64]
    assert f.num_rows == n and [g["rows"] for g in f.groups] == [1100, 1100, 800] and max(len(c["pages"]) for g in f.groups for c in g["chunks"]) > 1
    for (valid, values), (name, column) in zip(f.columns, cells.items()):
        present = [c for c in column if c is not None]
        assert valid.tolist() == [c is not None for c in column], name
        got = values.view("<i8").tolist() if name in "iz" else values if name == "s" else values.tolist()
        assert got == ([C.to_bits(c) for c in present] if name == "f" else [c.encode() for c in present] if name == "s" else present), name
