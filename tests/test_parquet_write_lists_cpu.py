"""The Parquet writer's list entries (oxh_write_parquet_lists_*) without a GPU: declared, exported and bound; their
argument errors in the header's order, before OXH_ERR_NODEVICE; the planner's level heads and list pages in a program of its own."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi

NAMES = ("oxh_write_parquet_lists_device", "oxh_write_parquet_lists_host")
LIST32 = _capi.OXH_PARQUET_LIST | _capi.OXH_CSV_INT32


def test_the_entries_are_declared_exported_and_bound(built_lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oxen_hash.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header and name in _capi.SIGNATURES and getattr(_capi.lib(), name).argtypes == _capi.SIGNATURES[name][1]
    assert len(_capi.SIGNATURES[NAMES[0]][1]) == len(_capi.SIGNATURES["oxh_write_parquet_device"][1]) + 2


def call(**change):
    """The host entry, NULL context, over one list<int32> column of three rows {[7, 8], null, []}; `change` replaces arguments."""
    u32s = lambda *v: (ctypes.c_uint32 * len(v))(*v)   # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)   # noqa: E731
    keep = [np.array([7, 8], dtype=np.int32), np.array([0, 2, 2, 2], dtype=np.int32), np.array([5], dtype=np.uint8), np.frombuffer(b"v\0", dtype=np.uint8),
            np.array([0, 1], dtype=np.uint64)]
    size, stats = ctypes.c_uint64(77), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    args = dict(ctx=None, nrows=3, ncols=1, types=u32s(LIST32), kinds=u32s(_capi.OXH_COL_FIXED4), values=ptrs(keep[0].ctypes.data),
                offsets=ptrs(keep[1].ctypes.data), validity=ptrs(keep[2].ctypes.data), bits=(ctypes.c_uint64 * 2)(), names=keep[3].ctypes.data,
                name_offsets=keep[4].ctypes.data_as(_capi._u64p), rows_per_group=0, page_bytes=0, flags=0, out=None, capacity=0,
                out_bytes=ctypes.byref(size), stats4=stats, child_validity=None, child_bits=None)
    for name, value in change.items():
        args[name] = value(keep) if callable(value) else value
    rc = _capi.lib().oxh_write_parquet_lists_host(*args.values())
    assert rc != _capi.OXH_OK and size.value == 77 and list(stats) == [7] * 4, "a refused call wrote an output"
    return rc, _capi.lib().oxh_last_error()


@pytest.mark.parametrize("change, what", [
    (dict(types=(ctypes.c_uint32 * 1)(_capi.OXH_PARQUET_LIST | _capi.OXH_CSV_STRING)), b"column 0 is a list of element type 4"),
    (dict(kinds=(ctypes.c_uint32 * 1)(_capi.OXH_COL_FIXED8)), b"has kind 8, not 4"),
    (dict(offsets=(ctypes.c_void_p * 1)(None)), b"column 0 is a list column without offsets"),
    (dict(offsets=lambda keep: (ctypes.c_void_p * 1)(keep[1].ctypes.data + 2)), b"list offsets are not aligned to 4 bytes"),
    (dict(offsets=lambda keep: (ctypes.c_void_p * 1)(keep.append(np.array([2, 0, 9, 9], dtype=np.int32)) or keep[-1].ctypes.data)), b"decrease or are negative at row 0"),
    (dict(values=(ctypes.c_void_p * 1)(None)), b"column 0 has elements but no values"),
], ids=["element", "kind", "no-offsets", "alignment", "pair", "no-values"])
def test_argument_errors_need_no_device(built_lib, change, what):
    rc, said = call(**change)
    assert rc == _capi.OXH_ERR_INVALID and said.startswith(b"parquet write:") and what in said, said
    # the first of them is named with every later one present too: a bad element word in front of NULL offsets and values
    if "types" in change:
        assert call(**change, offsets=(ctypes.c_void_p * 1)(None), values=(ctypes.c_void_p * 1)(None))[1] == said


def test_well_formed_lists_reach_the_device_check(built_lib):
    rc, said = call()
    assert rc == _capi.OXH_ERR_NODEVICE or b"ctx is NULL" in said, said


def test_native_program(built_lib, tmp_path):
    """The planner's level heads at 1, 7, 8 and 9 entries and its list pages, as build.py builds the program and under
    ASan / UBSan (a program of its own)."""
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_write_lists_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_WRITE_LISTS_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_WRITE_LISTS_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stderr for r in outs]
