"""OXH_PARQUET_INFLATE_ZSTD without a GPU: with the flag the footer of a ZSTD file passes and the open gets as far as
the device; bit 0 of the flags stays unknown; the size bound of a ZSTD page at its edge. zstd_tables.hpp's bit reader
and table builders in a program of their own, plain and under ASan / UBSan."""
import subprocess

import _parquet_cases as K
import test_parquet_read_cpu as P
from oxen_amd import _capi

ZSTD, SNAPPY = _capi.OXH_PARQUET_INFLATE_ZSTD, _capi.OXH_PARQUET_INFLATE


def test_zstd_flag_needs_no_device(built_lib):
    for name in ("zstd_v1_dict_fallback", "zstd_snappy_mixed"):
        data = K.fixture_bytes(name)
        for flags in (ZSTD | SNAPPY,) + ((ZSTD,) if "mixed" not in name else ()):   # the footer passes
            rc, msg, untouched = P.open_host(data, flags=flags)
            assert (rc == _capi.OXH_ERR_NODEVICE or "ctx is NULL" in msg) and untouched, msg
        for flags in (0, SNAPPY):
            rc, msg, untouched = P.open_host(data, flags=flags)
            assert rc == _capi.OXH_ERR_INVALID and "compression codec 6" in msg and untouched, msg
        for flags in (5, 7, 8):
            rc, msg, untouched = P.open_host(data, flags=flags)
            assert rc == _capi.OXH_ERR_INVALID and "unknown flags" in msg and untouched, msg
    rc, msg, untouched = P.open_host(K.fixture_bytes("zstd_snappy_mixed"), flags=ZSTD)   # its SNAPPY chunks need the other flag
    assert rc == _capi.OXH_ERR_INVALID and "compression codec 1" in msg and untouched, msg


def test_native_program(built_lib, tmp_path):
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "zstd_tables_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.ZSTD_TABLES_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.ZSTD_TABLES_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stdout + r.stderr for r in outs]
