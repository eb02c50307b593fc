"""What OXH_PARQUET_DICTIONARY needs no GPU for: the planner's dictionary chunks (tests/native/parquet_dict_host_test.cpp),
as build.py builds it and under the address and undefined-behaviour sanitizers."""
import subprocess


def test_native_program(built_lib, tmp_path):
    from oxen_amd import build

    build.build_host()
    exe = str(tmp_path / "parquet_dict_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.PARQUET_DICT_TEST_SRC], check=True, timeout=300)
    outs = [subprocess.run([prog], capture_output=True, text=True, timeout=300) for prog in (build.PARQUET_DICT_TEST, exe)]
    assert all(r.returncode == 0 and r.stdout.strip() == "ok" for r in outs), [r.stderr for r in outs]
