"""oxh_snappy_compress_* without a GPU: the bound's values, and the argument refusals in the header's order, every one
before the device is looked for."""
import ctypes
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi, tabular


def test_bound(built_lib):
    assert [tabular.snappy_bound(n) for n in (0, 1, 6, (1 << 32) - 1)] == [32, 33, 39, 32 + (1 << 32) - 1 + ((1 << 32) - 1) // 6]


def call(form, nblocks=1, src=True, src_offsets=(0, 10), dst=True, dst_offsets=(0, 100), sizes=True, status=True):
    lib = _capi.lib()
    buf = np.zeros(128, dtype=np.uint8)
    so, do = (None if a is None else np.array(a, dtype=np.uint64) for a in (src_offsets, dst_offsets))
    out_sizes, out_status = np.full(2, 99, dtype=np.uint64), np.full(2, 99, dtype=np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    args = [None, nblocks, ptr(buf) if src else None, ptr(so), ptr(buf) if dst else None, ptr(do), ptr(out_sizes) if sizes else None,
            ptr(out_status) if status else None]
    if form == "device":
        rc = lib.oxh_snappy_compress_device(*args, None)
    else:
        u64 = lambda a: None if a is None else ctypes.cast(a, _capi._u64p)  # noqa: E731
        args[3], args[5], args[6] = u64(args[3]), u64(args[5]), u64(args[6])
        args[7] = None if args[7] is None else ctypes.cast(args[7], ctypes.POINTER(ctypes.c_uint32))
        rc = lib.oxh_snappy_compress_host(*args)
    assert out_sizes[0] == 99 and out_status[0] == 99 and not buf.any()
    return rc, lib.oxh_last_error().decode()


@pytest.mark.parametrize("form", ["host", "device"])
def test_refusals_in_order(built_lib, form):
    assert call(form, nblocks=0, src=False, src_offsets=None, dst_offsets=None, sizes=False, status=False)[0] == _capi.OXH_OK
    broken = dict(src=False, src_offsets=None, dst_offsets=None, sizes=False, status=False, dst=False)
    steps = [(dict(nblocks=(1 << 32) + 1), "more than 2^32 blocks"), (dict(), "src is NULL"), (dict(src=True), "src_offsets is NULL"),
             (dict(src_offsets=(0, 1 << 32)), "dst_offsets is NULL"), (dict(dst_offsets=(0, 1 << 40)), "sizes is NULL"),
             (dict(sizes=True), "status is NULL"), (dict(status=True), "dst is NULL" if form == "device" else "block 0 has 4294967296 B"),
             (dict(src_offsets=(0, 10)), "dst is NULL")]
    for fix, message in steps:   # every step mends what the one before named
        rc, msg = call(form, **{**broken, **fix})
        assert rc == _capi.OXH_ERR_INVALID and msg.startswith("snappy compress: " + message), (fix, msg)
        broken.update({k: v for k, v in fix.items() if k != "nblocks"})
    rc, msg = call(form, **{**broken, "dst": True})   # nothing is left to refuse but the device, then the NULL ctx
    assert rc == _capi.OXH_ERR_NODEVICE or (rc == _capi.OXH_ERR_INVALID and msg == "snappy compress: ctx is NULL"), (rc, msg)


def test_the_parquet_writers_flag_needs_no_device(built_lib):
    """OXH_PARQUET_SNAPPY passes the flag check and the call gets as far as the device; bit 0 stays unknown."""
    import _csvwrite_call as C

    cols, types, _ = C.refusal_frame()
    tables = tabular._tables(cols, lambda a: None if a is None else a.ctypes.data)
    n = len(cols)
    offsets, names = np.arange(n + 1, dtype=np.uint64), np.frombuffer(b"ifbsS\0", dtype=np.uint8)
    size, stats = ctypes.c_uint64(77), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    lib = _capi.lib()
    for flags, want in ((2, None), (1, b"unknown flags"), (3, b"unknown flags")):
        rc = lib.oxh_write_parquet_host(None, 3, n, (ctypes.c_uint32 * n)(*types), *tables, names.ctypes.data, offsets.ctypes.data_as(_capi._u64p), 0, 0,
                                        flags, None, 0, ctypes.byref(size), stats)
        msg = lib.oxh_last_error()
        assert (rc == _capi.OXH_ERR_INVALID and want in msg) if want else rc == _capi.OXH_ERR_NODEVICE or (rc == _capi.OXH_ERR_INVALID and msg == b"ctx is NULL"), (flags, rc, msg)
        assert size.value == 77 and list(stats) == [7] * 4


def test_compression_names(built_lib):
    import _csvwrite_call as C

    frame = {"a": C.host_column(C.W.INT64, [1, 2, 3])}
    for form in (tabular.write_parquet, tabular.write_parquet_device):
        with pytest.raises(_capi.OxenError, match="compression 'zstd'"):
            form(frame, compression="zstd")


def test_native_program(built_lib, tmp_path):
    """parquet_host.hpp's plan with stored sizes and snappy_capacity() in a program of their own, plain and under ASan / UBSan."""
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_snappy_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_SNAPPY_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_SNAPPY_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stderr for r in outs]
