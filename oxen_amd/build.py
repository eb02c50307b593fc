"""Build the in-tree HIP library (oxen_amd/liboxen_hash.so) for gfx950 with hipcc.

The .so is git-ignored but travels to the GPU box with the repo snapshot; no JIT cache is used.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "liboxen_hash.so")
# the C ABI runtime (capi_internal.hpp lists its pieces), the kernels, FastCDC, the reader pool, RCCL
SOURCES = [os.path.join(CSRC, f) for f in (
    "xxh3_kernels.hip", "capi_dispatch.hip", "capi_context.hip", "staging.hip", "large_items.hip", "xxh3_stream.hip",
    "engine.hip", "modified.hip", "publish.hip", "fastcdc.hip", "fastcdc_scan.hip", "fastcdc_walk.hip", "dedup_index.hip",
    "row_hash.hip", "keyed_diff.hip", "take_columns.hip", "concat_columns.hip", "sort_rows.hip", "group_rows.hip", "filter_rows.hip",
    "embedding.hip", "csv_read.hip", "csv_write.hip", "json_write.hip", "jsonl_read.hip", "reader_pool.cpp", "comm.cpp", "fastcdc_host.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, h) for h in ("capi_internal.hpp", "xxh3_device.hpp", "fastcdc_gear.h", "fastcdc_plan.hpp",
                                                 "fastcdc_device.hpp", "pool.hpp", "scratch.hpp", "reader_pool.hpp",
                                                 "env.hpp", "keyed_diff_host.hpp", "columns.hpp",
                                                 "take_columns_host.hpp", "concat_columns_host.hpp", "sort_rows_host.hpp", "sort_keys.hpp",
                                                 "group_rows_host.hpp", "filter_rows_host.hpp", "filter_terms.hpp",
                                                 "embedding_host.hpp", "csv_host.hpp", "csv_number.hpp", "csv_text.hpp", "json_text.hpp", "jsonl_host.hpp",
                                                 "jsonl_text.hpp")] + [os.path.join(ROOT, "include", "oxen_hash.h")]
HELPER_SRC = os.path.join(CSRC, "hash_helper.cpp")
HELPER = os.path.join(HERE, "oxh_hash_helper")  # the reader-pool helper process (oxh_pool_*)
ARCH = "gfx950"


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (expected /opt/rocm/bin/hipcc)")


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in DEPS)


HOST_SRC = os.path.join(HERE, "host", "oxen_hasher.cpp")
HOST_HDR = os.path.join(HERE, "host", "oxen_hasher.hpp")
COMMIT_SRC = os.path.join(HERE, "host", "commit_writer.cpp")
COMMIT_HDR = os.path.join(HERE, "host", "commit_writer.hpp")
HOST_LIB = os.path.join(HERE, "liboxen_hasher.so")
NATIVE_TEST_SRC = os.path.join(ROOT, "tests", "native", "test_hasher.cpp")
NATIVE_TEST = os.path.join(ROOT, "tests", "native", "test_hasher")
COMMIT_CLI_SRC = os.path.join(ROOT, "tests", "native", "commit_tree_cli.cpp")
COMMIT_CLI = os.path.join(ROOT, "tests", "native", "commit_tree_cli")
FAKE_HELPER_SRC = os.path.join(ROOT, "tests", "native", "fake_pool_helper.cpp")
FAKE_HELPER = os.path.join(ROOT, "tests", "native", "fake_pool_helper")  # tests only: the pool without a GPU
C_CONSUMER_SRC = os.path.join(ROOT, "tests", "native", "abi_c_consumer.c")
C_CONSUMER = os.path.join(ROOT, "tests", "native", "abi_c_consumer")  # tests only: a plain C99 caller of the ABI
PLAN_TEST_SRC = os.path.join(ROOT, "tests", "native", "cdc_plan_test.cpp")
PLAN_TEST = os.path.join(ROOT, "tests", "native", "cdc_plan_test")  # tests only: the FastCDC planner on the CPU
KEYED_TEST_SRC = os.path.join(ROOT, "tests", "native", "keyed_diff_host_test.cpp")
KEYED_TEST = os.path.join(ROOT, "tests", "native", "keyed_diff_host_test")  # tests only: the keyed diff's host pieces
TAKE_TEST_SRC = os.path.join(ROOT, "tests", "native", "take_columns_host_test.cpp")
TAKE_TEST = os.path.join(ROOT, "tests", "native", "take_columns_host_test")  # tests only: the take's host pieces
CONCAT_TEST_SRC = os.path.join(ROOT, "tests", "native", "concat_columns_host_test.cpp")
CONCAT_TEST = os.path.join(ROOT, "tests", "native", "concat_columns_host_test")  # tests only: the concat's host pieces
SORT_TEST_SRC = os.path.join(ROOT, "tests", "native", "sort_rows_host_test.cpp")
SORT_TEST = os.path.join(ROOT, "tests", "native", "sort_rows_host_test")  # tests only: the row sort's host pieces and key words
GROUP_TEST_SRC = os.path.join(ROOT, "tests", "native", "group_rows_host_test.cpp")
GROUP_TEST = os.path.join(ROOT, "tests", "native", "group_rows_host_test")  # tests only: the grouping's host pieces
FILTER_TEST_SRC = os.path.join(ROOT, "tests", "native", "filter_rows_host_test.cpp")
FILTER_TEST = os.path.join(ROOT, "tests", "native", "filter_rows_host_test")  # tests only: the filter's terms and host pieces
EMBEDDING_TEST_SRC = os.path.join(ROOT, "tests", "native", "embedding_host_test.cpp")
EMBEDDING_TEST = os.path.join(ROOT, "tests", "native", "embedding_host_test")  # tests only: the embedding query's host pieces and order key
CSV_TEST_SRC = os.path.join(ROOT, "tests", "native", "csv_host_test.cpp")
CSV_TEST = os.path.join(ROOT, "tests", "native", "csv_host_test")  # tests only: the CSV reader's parsers and host pieces
CSV_WRITE_TEST_SRC = os.path.join(ROOT, "tests", "native", "csv_write_host_test.cpp")
CSV_WRITE_TEST = os.path.join(ROOT, "tests", "native", "csv_write_host_test")  # tests only: the CSV writer's text functions
CSV_FLOAT_CASES_SRC = os.path.join(ROOT, "tests", "native", "csv_float_cases.cpp")
CSV_FLOAT_CASES = os.path.join(ROOT, "tests", "native", "csv_float_cases")  # tests only: both CSV float conversions over a test's cells
JSON_WRITE_TEST_SRC = os.path.join(ROOT, "tests", "native", "json_write_host_test.cpp")
JSON_WRITE_TEST = os.path.join(ROOT, "tests", "native", "json_write_host_test")  # tests only: the JSON writer's text functions
JSONL_TEST_SRC = os.path.join(ROOT, "tests", "native", "jsonl_host_test.cpp")
JSONL_TEST = os.path.join(ROOT, "tests", "native", "jsonl_host_test")  # tests only: the JSON Lines reader's grammar, carries and host pieces
FAKE_RCCL_SRC = os.path.join(ROOT, "tests", "native", "fake_rccl.cpp")
# tests only: an "RCCL" for N processes on one GPU (OXH_RCCL_LIB), with and without ncclGather
FAKE_RCCL = os.path.join(ROOT, "tests", "native", "libfake_rccl.so")
FAKE_RCCL_NOGATHER = os.path.join(ROOT, "tests", "native", "libfake_rccl_nogather.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _stale(target: str, deps: list[str]) -> bool:
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def build_host(force: bool = False, verbose: bool = False) -> str:
    """The C++ host mirror over the C ABI (oxen_amd/host, g++): liboxen `util::hasher` + MerkleHash
    and the commit writer's K2 driver, in liboxen_hasher.so; its native test programs
    (tests/native/test_hasher.cpp, commit_tree_cli.cpp), which link against liboxen_hash.so; and the
    stand-alone CPU tests of the FastCDC planner (tests/native/cdc_plan_test.cpp), of the keyed diff's
    host pieces (tests/native/keyed_diff_host_test.cpp), of the take's (tests/native/take_columns_host_test.cpp), of
    the concat's (tests/native/concat_columns_host_test.cpp), of the row sort's host pieces and key words (tests/native/sort_rows_host_test.cpp), of the grouping's host pieces
    (tests/native/group_rows_host_test.cpp), of the filter's terms and host pieces
    (tests/native/filter_rows_host_test.cpp), of the embedding query's host pieces and order key
    (tests/native/embedding_host_test.cpp), of the CSV reader's parsers and host pieces
    (tests/native/csv_host_test.cpp), of the CSV writer's text functions (tests/native/csv_write_host_test.cpp), of
    both CSV float conversions over cells a test sends in (tests/native/csv_float_cases.cpp), of the JSON writer's
    text functions (tests/native/json_write_host_test.cpp) and of the JSON Lines reader's grammar, carries and host
    pieces (tests/native/jsonl_host_test.cpp)."""
    hdr = os.path.join(ROOT, "include", "oxen_hash.h")
    steps = [
        (HELPER, [HELPER_SRC, os.path.join(CSRC, "reader_pool.hpp"), hdr, LIB],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", HELPER + ".tmp", HELPER_SRC,
          f"-L{HERE}", "-l:liboxen_hash.so", "-Wl,-rpath,$ORIGIN"]),
        (HOST_LIB, [HOST_SRC, HOST_HDR, COMMIT_SRC, COMMIT_HDR, hdr, LIB],
         ["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", HOST_LIB + ".tmp", HOST_SRC, COMMIT_SRC,
          f"-L{HERE}", "-l:liboxen_hash.so", "-Wl,-rpath,$ORIGIN"]),
        (NATIVE_TEST, [NATIVE_TEST_SRC, HOST_HDR, HOST_LIB],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", NATIVE_TEST + ".tmp", NATIVE_TEST_SRC,
          f"-L{HERE}", "-l:liboxen_hasher.so", "-l:liboxen_hash.so", "-Wl,-rpath,$ORIGIN/../../oxen_amd"]),
        (FAKE_HELPER, [FAKE_HELPER_SRC, os.path.join(CSRC, "reader_pool.hpp")],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", FAKE_HELPER + ".tmp", FAKE_HELPER_SRC]),
        (C_CONSUMER, [C_CONSUMER_SRC, hdr, LIB],
         ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-o", C_CONSUMER + ".tmp", C_CONSUMER_SRC,
          f"-L{HERE}", "-l:liboxen_hash.so", "-Wl,-rpath,$ORIGIN/../../oxen_amd"]),
        (COMMIT_CLI, [COMMIT_CLI_SRC, COMMIT_HDR, HOST_HDR, HOST_LIB],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", COMMIT_CLI + ".tmp", COMMIT_CLI_SRC,
          f"-L{HERE}", "-l:liboxen_hasher.so", "-l:liboxen_hash.so", "-Wl,-rpath,$ORIGIN/../../oxen_amd"]),
        (PLAN_TEST, [PLAN_TEST_SRC, os.path.join(CSRC, "fastcdc_plan.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", PLAN_TEST + ".tmp", PLAN_TEST_SRC]),
        (KEYED_TEST, [KEYED_TEST_SRC, os.path.join(CSRC, "keyed_diff_host.hpp")],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", KEYED_TEST + ".tmp", KEYED_TEST_SRC]),
        (TAKE_TEST, [TAKE_TEST_SRC, os.path.join(CSRC, "take_columns_host.hpp"), os.path.join(CSRC, "columns.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", TAKE_TEST + ".tmp", TAKE_TEST_SRC]),
        (CONCAT_TEST, [CONCAT_TEST_SRC, os.path.join(CSRC, "concat_columns_host.hpp"), os.path.join(CSRC, "columns.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", CONCAT_TEST + ".tmp", CONCAT_TEST_SRC]),
        (SORT_TEST, [SORT_TEST_SRC, os.path.join(CSRC, "sort_rows_host.hpp"), os.path.join(CSRC, "sort_keys.hpp"),
                     os.path.join(CSRC, "columns.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", SORT_TEST + ".tmp", SORT_TEST_SRC]),
        (GROUP_TEST, [GROUP_TEST_SRC, os.path.join(CSRC, "group_rows_host.hpp"), os.path.join(CSRC, "sort_rows_host.hpp"),
                      os.path.join(CSRC, "sort_keys.hpp"), os.path.join(CSRC, "columns.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", GROUP_TEST + ".tmp", GROUP_TEST_SRC]),
        (FILTER_TEST, [FILTER_TEST_SRC, os.path.join(CSRC, "filter_rows_host.hpp"), os.path.join(CSRC, "filter_terms.hpp"),
                       os.path.join(CSRC, "sort_rows_host.hpp"), os.path.join(CSRC, "sort_keys.hpp"), os.path.join(CSRC, "columns.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", FILTER_TEST + ".tmp", FILTER_TEST_SRC]),
        (EMBEDDING_TEST, [EMBEDDING_TEST_SRC, os.path.join(CSRC, "embedding_host.hpp"), os.path.join(CSRC, "sort_keys.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", EMBEDDING_TEST + ".tmp", EMBEDDING_TEST_SRC]),
        (CSV_TEST, [CSV_TEST_SRC, os.path.join(CSRC, "csv_host.hpp"), os.path.join(CSRC, "csv_number.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", CSV_TEST + ".tmp", CSV_TEST_SRC]),
        (CSV_WRITE_TEST, [CSV_WRITE_TEST_SRC, os.path.join(CSRC, "csv_text.hpp")],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", CSV_WRITE_TEST + ".tmp", CSV_WRITE_TEST_SRC]),
        (CSV_FLOAT_CASES, [CSV_FLOAT_CASES_SRC, os.path.join(CSRC, "csv_host.hpp"), os.path.join(CSRC, "csv_number.hpp"),
                           os.path.join(CSRC, "csv_text.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", CSV_FLOAT_CASES + ".tmp", CSV_FLOAT_CASES_SRC]),
        (JSON_WRITE_TEST, [JSON_WRITE_TEST_SRC, os.path.join(CSRC, "json_text.hpp"), os.path.join(CSRC, "csv_text.hpp")],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", JSON_WRITE_TEST + ".tmp", JSON_WRITE_TEST_SRC]),
        (JSONL_TEST, [JSONL_TEST_SRC, os.path.join(CSRC, "jsonl_host.hpp"), os.path.join(CSRC, "jsonl_text.hpp"),
                      os.path.join(CSRC, "csv_host.hpp"), os.path.join(CSRC, "csv_number.hpp"), hdr],
         ["g++", "-std=c++17", "-O2", "-Wall", "-o", JSONL_TEST + ".tmp", JSONL_TEST_SRC]),
    ]
    for target, extra in ((FAKE_RCCL, []), (FAKE_RCCL_NOGATHER, ["-DFAKE_NO_GATHER"])):
        steps.append((target, [FAKE_RCCL_SRC],
                      ["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-fvisibility=hidden",
                       "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", "-o", target + ".tmp", FAKE_RCCL_SRC] + extra +
                      [f"-L{ROCM}/lib", "-lamdhip64", "-lrt", f"-Wl,-rpath,{ROCM}/lib"]))
    tests_native = os.path.join(ROOT, "tests", "native") + os.sep
    for target, deps, cmd in steps:
        # a test program is built where its source is: the package builds beside any tests/ tree, or none
        if deps[0].startswith(tests_native) and not os.path.exists(deps[0]):
            continue
        if force or _stale(target, deps):
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.run(cmd, check=True)
            os.replace(target + ".tmp", target)
    return HOST_LIB


def compile_lib(out: str, verbose: bool = False) -> str:
    """hipcc every source to its own object in parallel (one hipcc per source), then link `out`."""
    from concurrent.futures import ThreadPoolExecutor

    objdir = os.path.join(HERE, "build", os.path.basename(out).replace(".so", ""))
    os.makedirs(objdir, exist_ok=True)
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall"]

    def one(src: str) -> str:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        cmd = [hipcc()] + flags + ["-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        return obj

    jobs = max(1, min(len(SOURCES), int(os.environ.get("MAX_JOBS", "0") or 0) or (os.cpu_count() or 4)))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(one, SOURCES))
    tmp = out + ".tmp"
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-Wl,--no-undefined", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        build_host(verbose=verbose)
        return LIB
    compile_lib(LIB, verbose=verbose)
    build_host(force=True, verbose=verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
