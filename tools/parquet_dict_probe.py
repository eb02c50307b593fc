"""OXH_PARQUET_DICTIONARY (`write_parquet_device(..., dictionary=True)`, oxen_amd/csrc/parquet_dict.hip) at the size of a
real table: --rows (10 M) rows of tools/csv_probe.py's five-column shape, whose fourth column is a string of 100 labels.
It records, and fixes nothing in advance:
  table   the file's size and the device form's time with the flag off and on, alone and with SNAPPY, alternated in one
          loop so that all four see the same machine (the flag off is the PLAIN writer as it was); the dictionary file
          read back by `read_parquet` and compared with the PLAIN file's columns before anything is timed; and
          pyarrow's `write_table(use_dictionary=True)` of the same table on 16 threads, uncompressed and with SNAPPY,
          when pyarrow imports (without it the probe says so and leaves that out);
  steps   per arm of the insert's LDS first level (OXH_PQD_LDS_LEVEL 1 and 0), a library built from parquet_dict.hip
          with OXH_PQD_STEP_EVENTS, which times insert, rank, gather and pack by events: the table, the label column
          alone, and a column of all-distinct int64 alone.
Every part runs in a process of its own under a time limit. Two warm calls, medians of --reps, a host clock around calls
that block until the device is done.

    python tools/parquet_dict_probe.py [--rows 10000000] [--reps 5] [--out profiles/parquet_dict/probe.json]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from csv_probe import five_columns  # noqa: E402
from json_write_probe import alternated  # noqa: E402

ARMS = (1, 0)  # OXH_PQD_LDS_LEVEL


def build_arm(lds: int, arms_dir: str) -> str:
    """The library with parquet_dict.hip rebuilt for one arm, with the step events (the other objects are the main build's)."""
    from oxen_amd import build

    out = os.path.join(arms_dir, "liboxen_hash_pqd_lds%d_events.so" % lds)
    src = os.path.join(build.CSRC, "parquet_dict.hip")
    if os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(src):
        return out
    objdir = os.path.join(build.HERE, "build", "liboxen_hash")
    objs = [os.path.join(objdir, os.path.basename(f) + ".o") for f in build.SOURCES]
    if not all(os.path.exists(o) for o in objs):
        build.compile_lib(build.LIB)
    os.makedirs(arms_dir, exist_ok=True)
    mine = out[:-3] + ".o"
    subprocess.run([build.hipcc(), "--offload-arch=" + build.ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-DOXH_PQD_LDS_LEVEL=%d" % lds,
                    "-DOXH_PQD_STEP_EVENTS=1", "-c", "-o", mine, src], check=True)
    subprocess.run([build.hipcc(), "--offload-arch=" + build.ARCH, "-shared", "-fPIC", "-Wl,--no-undefined", "-o", out] +
                   [mine if o.endswith("parquet_dict.hip.o") else o for o in objs], check=True)
    return out


def table_part(a, torch, tabular, ctx, d_frame) -> dict:
    write = lambda **kw: tabular.write_parquet_device(d_frame, ctx=ctx, stream=ctx.stream, **kw)  # noqa: E731
    arms = {"plain": {}, "dictionary": {"dictionary": True}, "plain_snappy": {"compression": "snappy"},
            "dictionary_snappy": {"compression": "snappy", "dictionary": True}}
    files = {name: write(**kw).cpu().numpy().tobytes() for name, kw in arms.items()}
    want = tabular.read_parquet(files["plain"], ctx=ctx)
    for name in ("dictionary", "dictionary_snappy"):
        got = tabular.read_parquet(files[name], ctx=ctx)
        for key in want:
            for x, y in zip((want[key].values, want[key].offsets, want[key].validity), (got[key].values, got[key].offsets, got[key].validity)):
                assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)), (name, key)
    out = alternated({name: (lambda kw=kw: write(**kw)) for name, kw in arms.items()}, a.reps)
    for name in arms:
        out[name]["file_bytes"] = len(files[name])
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq
    except ImportError:
        out["pyarrow"] = "not installed: not measured"
        return out
    pa.set_cpu_count(16)
    table = pq.read_table(io.BytesIO(files["plain"]))

    def theirs(codec):
        sink = io.BytesIO()
        pq.write_table(table, sink, use_dictionary=True, compression=codec)
        return sink.tell()

    out["pyarrow_use_dictionary_16_threads"] = alternated({"none": lambda: theirs("NONE"), "snappy": lambda: theirs("SNAPPY")}, a.reps)
    out["pyarrow_use_dictionary_16_threads"]["none"]["file_bytes"] = theirs("NONE")
    out["pyarrow_use_dictionary_16_threads"]["snappy"]["file_bytes"] = theirs("SNAPPY")
    return out


def steps_part(a, torch, tabular, ctx, d_frame) -> dict:
    """A child with an arm's library: it only runs the calls; their PQD_STEPS lines on stderr are the parent's to read."""
    from oxen_amd import _capi

    distinct = {"k": tabular.Column(8, a.rows, torch.arange(a.rows, dtype=torch.int64, device="cuda:0"))}
    frames = {"table": (d_frame, None), "label_alone": ({"label": d_frame["label"]}, None), "distinct_int64_alone": (distinct, [_capi.OXH_CSV_INT64])}
    for name, (frame, types) in frames.items():
        for _ in range(2 + a.reps):
            print("PQD_FRAME " + name, file=sys.stderr, flush=True)
            tabular.write_parquet_device(frame, types=types, ctx=ctx, stream=ctx.stream, dictionary=True)
    return {}


def steps_of(stderr: str, reps: int) -> dict:
    runs, frame = {}, None
    for line in stderr.splitlines():
        if line.startswith("PQD_FRAME "):
            frame = line[10:]
        elif line.startswith("PQD_STEPS ") and frame:
            runs.setdefault(frame, []).append(json.loads(line[10:]))
    # a frame none of whose chunks got a dictionary (the distinct column) has no gather and no pack: they are 0
    return {f: {k: round(statistics.median(x[k] for x in r[-reps:]), 3) for k in r[0]} for f, r in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parquet_dict", "probe.json"))
    ap.add_argument("--arms-dir", default=os.path.join(ROOT, "oxen_amd", "build", "arms"))
    ap.add_argument("--build-arms", action="store_true", help="only build the arms' libraries (needs no GPU)")
    ap.add_argument("--part", choices=("table", "steps"), help="a child of this probe: one part, as one JSON line")
    ap.add_argument("--arm-lib")
    a = ap.parse_args()
    if a.build_arms:
        print([build_arm(lds, a.arms_dir) for lds in ARMS])
        return
    if a.part:
        import torch

        from oxen_amd import _capi, tabular

        if not torch.cuda.is_available():
            sys.exit("parquet_dict_probe: no GPU (there is nothing to measure on a CPU)")
        if a.arm_lib:
            _capi.LIB_PATH = a.arm_lib
        ctx = _capi.Context(0)
        data, rows = five_columns(np.random.default_rng(a.seed), a.rows)
        d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        d_frame = tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream)
        del d
        print("PART " + json.dumps((table_part if a.part == "table" else steps_part)(a, torch, tabular, ctx, d_frame)), flush=True)
        return

    def child(part, lib=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--reps", str(a.reps), "--seed", str(a.seed), "--part", part]
        run = subprocess.run(cmd + (["--arm-lib", lib] if lib else []), capture_output=True, text=True, timeout=420)
        line = [x for x in run.stdout.splitlines() if x.startswith("PART ")]
        if run.returncode or not line:
            sys.exit("parquet_dict_probe: part %s (%s) ended with %d: %s" % (part, lib, run.returncode, run.stderr[-800:]))  # nothing more is started
        return json.loads(line[0][5:]), run.stderr

    out = {"rows": a.rows, "reps": a.reps, "table": child("table")[0], "steps_by_events": {}}
    print("table", json.dumps(out["table"]), flush=True)
    for lds in ARMS:
        out["steps_by_events"]["lds_level_%d" % lds] = steps_of(child("steps", build_arm(lds, a.arms_dir))[1], a.reps)
        print(lds, json.dumps(out["steps_by_events"]["lds_level_%d" % lds]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
