"""The Parquet reader's list columns without a GPU: a list fixture now passes the host form's footer checks, which come
before OXH_ERR_NODEVICE; a struct column is still refused at open and a list of strings passes the footer (it is the
column's own refusal); the entry's argument checks need no device; parquet_read_host.hpp's list planning in a program
of its own, plain and under ASan / UBSan, which also counts the fixtures' pages that begin in the middle of a row."""
import ctypes
import os
import subprocess

import pytest

from oxen_amd import _capi
from test_parquet_read_cpu import GOLDEN, open_host


def fixture(name):
    with open(os.path.join(GOLDEN, name + ".parquet"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", ["lists_v1", "lists_v2_zstd", "lists_split_rows", "list_of_strings"])
def test_a_list_file_passes_the_footer(built_lib, name):
    rc, msg, untouched = open_host(fixture(name), flags=_capi.OXH_PARQUET_INFLATE | _capi.OXH_PARQUET_INFLATE_ZSTD)
    assert (rc == _capi.OXH_ERR_NODEVICE or "ctx is NULL" in msg) and untouched, msg


def test_what_is_still_refused_at_open(built_lib):
    rc, msg, untouched = open_host(fixture("nested_struct"))
    assert rc == _capi.OXH_ERR_INVALID and "parquet open: column 'st' is a nested field (a group of 2)" in msg and untouched, msg
    good = fixture("lists_v1")
    i = good.index(b"\x18\x04li64")   # the list group's name in the footer; in front of it its repetition type, behind it num_children and the LIST annotations
    assert good[i - 2:i] == b"\x35\x02"
    rc, msg, _ = open_host(good[:i - 1] + b"\x04" + good[i:])   # OPTIONAL -> REPEATED
    assert rc == _capi.OXH_ERR_INVALID and "column 'li64' is a nested field" in msg, msg
    L, words = _capi.lib(), (ctypes.c_uint64 * 4)()
    assert L.oxh_parquet_lists_host(None, 0, None, None, None, None, None, None, None, words, words) == _capi.OXH_ERR_INVALID
    assert L.oxh_last_error().startswith(b"parquet lists: the handle is NULL")
    assert L.oxh_abi_version() == 5


def test_native_program(built_lib, tmp_path):
    """parquet_read_host.hpp's list planning as build.py builds it and under ASan / UBSan (a program of its own);
    pyarrow's V1 file has no page that begins in the middle of a row, the hand-cut one has 9 of 15."""
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_lists_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_LISTS_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_LISTS_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stderr for r in outs]
    counts = [subprocess.run([exe, os.path.join(GOLDEN, name + ".parquet")], capture_output=True, text=True, timeout=300).stdout.strip()
              for name in ("lists_v1", "lists_v2", "lists_split_rows")]
    assert counts == ["0", "0", "9"], counts
