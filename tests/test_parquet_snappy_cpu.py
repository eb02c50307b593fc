"""OXH_PARQUET_INFLATE without a GPU: with the flag the footer of a SNAPPY file passes and the open gets as far as the
device; every other codec is still refused by number; bit 0 of the flags stays unknown. parquet_read_host.hpp's codec
acceptance, size rule and image plan in a program of their own, plain and under ASan / UBSan."""
import subprocess

import test_parquet_read_cpu as P
from oxen_amd import _capi

INFLATE = _capi.OXH_PARQUET_INFLATE


def with_codec(byte):   # test_parquet_read_cpu's patch: column i32 of row group 0
    with open(P.os.path.join(P.GOLDEN, "v1_dict_fallback.parquet"), "rb") as f:
        good = f.read()
    at = good.index(b"\x18\x03i32\x15\x00") + 6
    return good[:at] + bytes([byte]) + good[at + 1:]


def test_inflate_flag_needs_no_device(built_lib):
    rc, msg, untouched = P.open_host(with_codec(0x02), flags=INFLATE)   # SNAPPY: the footer passes
    assert (rc == _capi.OXH_ERR_NODEVICE or "ctx is NULL" in msg) and untouched, msg
    for byte, number in ((0x04, 2), (0x0C, 6)):   # zigzag of GZIP and of ZSTD
        for flags in (0, INFLATE):
            rc, msg, untouched = P.open_host(with_codec(byte), flags=flags)
            assert rc == _capi.OXH_ERR_INVALID and "column 'i32': compression codec %d" % number in msg and untouched, msg
    for flags in (1, 3):
        rc, msg, untouched = P.open_host(with_codec(0x02), flags=flags)
        assert rc == _capi.OXH_ERR_INVALID and "unknown flags" in msg and untouched, msg


def test_native_program(built_lib, tmp_path):
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_inflate_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_INFLATE_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_INFLATE_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stderr for r in outs]
