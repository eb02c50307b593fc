"""The Parquet reader (oxh_parquet_*) without a GPU: the open's argument refusals in the header's order and the
footer's refusals through the host form, all before OXH_ERR_NODEVICE; parquet_bits.hpp and parquet_read_host.hpp in a
program of their own, plain and under ASan / UBSan (a nested schema element, which no overwritten byte of a fixture
makes, is a footer that program builds)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet")


def open_host(data, flags=0, out=True, stats=True, null_bytes=False):
    """(return code, message, whether the outputs are untouched) of oxh_parquet_open_host with a NULL context."""
    buf = np.frombuffer(data, dtype=np.uint8)
    handle, stats8 = ctypes.c_void_p(77), (ctypes.c_uint64 * 8)(*[7] * 8)
    rc = _capi.lib().oxh_parquet_open_host(None, None if null_bytes else buf.ctypes.data, buf.size, flags, ctypes.byref(handle) if out else None,
                                           stats8 if stats else None)
    return rc, _capi.lib().oxh_last_error().decode(), handle.value == 77 and list(stats8) == [7] * 8


def test_open_refusals_need_no_device(built_lib):
    """Each argument refusal with every later one present names the first; then the footer's, on patched copies of a
    fixture; nothing writes an output; the untouched file passes them all."""
    with open(os.path.join(GOLDEN, "v1_dict_fallback.parquet"), "rb") as f:
        good = f.read()
    faults = [(dict(flags=1), "unknown flags"), (dict(null_bytes=True), "bytes is NULL"), (dict(out=False), "out is NULL"), (dict(stats=False), "stats8 is NULL")]
    for k, (change, what) in enumerate(faults):
        later = {}
        for more, _ in reversed(faults[k + 1:]):
            later.update(more)
        rc, msg, untouched = open_host(b"not a parquet file", **{**later, **change})
        assert rc == _capi.OXH_ERR_INVALID and msg.startswith("parquet open:") and what in msg and untouched, (k, msg)

    def patched(find, at, byte):
        i = good.index(find)
        assert good.count(find) >= 1 and good[i + at] != byte
        return good[:i + at] + bytes([byte]) + good[i + at + 1:]

    size = len(good)
    footers = [(good[:11], "11 bytes"), (good[:-1] + b"2", "does not end with the magic PAR1"), (b"PAR2" + good[4:], "does not start with the magic PAR1"),
               (good[:-4] + b"PARE", "encrypted"), (good[:-8] + (size - 11).to_bytes(4, "little") + good[-4:], "a footer of %d bytes in a file of %d" % (size - 11, size)),
               (good[:-8 - 1] + b"\x15" + good[-8:], "not a FileMetaData"),
               (patched(b"\x25\x02\x18\x03i32", 1, 0x04), "column 'i32' is a repeated field"),                 # OPTIONAL -> REPEATED
               (patched(b"\x18\x03i32\x15\x00", 6, 0x02), "column 'i32': compression codec 1"),               # UNCOMPRESSED -> SNAPPY, row group 0
               (good[:100] + good[101:], "is not inside the file")]   # a byte less in front of the footer: the last chunk ends in it
    for data, what in footers:
        rc, msg, untouched = open_host(data)
        assert rc == _capi.OXH_ERR_INVALID and msg.startswith("parquet open:") and what in msg and untouched, (what, msg)
    rc, msg, untouched = open_host(good)
    assert (rc == _capi.OXH_ERR_NODEVICE or "ctx is NULL" in msg) and untouched, msg
    L, words = _capi.lib(), (ctypes.c_uint64 * 4)()
    assert L.oxh_parquet_close(None) == _capi.OXH_OK
    assert L.oxh_parquet_columns_host(None, 0, None, None, None, None, None, None, words, words) == _capi.OXH_ERR_INVALID
    assert L.oxh_last_error().startswith(b"parquet columns:") and L.oxh_parquet_types(None, None) == _capi.OXH_ERR_INVALID


def test_native_program(built_lib, tmp_path):
    """parquet_bits.hpp and parquet_read_host.hpp as build.py builds them and under ASan / UBSan (a program of its own)."""
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_read_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_READ_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_READ_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stderr for r in outs]
