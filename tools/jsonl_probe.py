"""The JSON Lines reader (oxh_jsonl_*) at the size of a real table: --rows (10 M) rows of the five-column frame of
the CSV and JSON probes (Int64, Float64, Boolean, two short strings), as the JSON Lines text `write_jsonl_device`
makes of the frame `read_csv_device` reads. It records, and fixes nothing in advance:
  device   the bytes already in HBM, with device events: the open (the index, the names) and the five columns as
           their inferred types (measure, output allocation and write, as `JsonlFile.columns` does them), separately;
           beside them in the same loop a plain device read of the same bytes (`torch.sum`) as the floor, and
           `oxh_csv_open_device` plus its columns on the same frame's CSV text;
  host     the host form end to end (`read_jsonl` from host bytes) on --host-rows rows, beside `json.loads` per line
           of the same bytes in the same run.
Two warm rounds, medians of --reps, the calls alternated in one loop.

    python tools/jsonl_probe.py [--rows 10000000] [--host-rows 1000000] [--reps 5] [--out profiles/jsonl/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jsonl", "probe.json"))
    args = ap.parse_args()
    import torch

    import csv_probe
    from oxen_amd import _capi, tabular

    ctx = _capi.Context(0)
    rng = np.random.default_rng(7)
    csv_bytes, rows = csv_probe.five_columns(rng, args.rows)
    d_csv = torch.from_numpy(np.frombuffer(csv_bytes, dtype=np.uint8).copy()).cuda()
    frame = tabular.read_csv_device(d_csv, ctx=ctx)
    d_jsonl = tabular.write_jsonl_device(frame, ctx=ctx)
    del frame
    torch.cuda.synchronize()

    def jsonl_open():
        return tabular.JsonlFile(d_jsonl, ctx=ctx, device=True)

    def csv_open():
        return tabular.CsvFile(d_csv, ctx=ctx, device=True)

    with jsonl_open() as f:
        stats, names, jsonl_types = f.stats, f.names, f.infer()
    with csv_open() as f:
        csv_types = f.infer()
    samples = {k: [] for k in ("jsonl_open", "jsonl_columns", "read_floor", "csv_open", "csv_columns")}
    for rep in range(args.reps + 2):
        ms, f = timed(jsonl_open)
        ms_cols, _ = timed(lambda: f.columns(list(range(len(names))), jsonl_types))
        f.close()
        ms_floor, _ = timed(lambda: torch.sum(d_jsonl, dtype=torch.int64))
        ms_csv, g = timed(csv_open)
        ms_csv_cols, _ = timed(lambda: g.columns(list(range(len(csv_types))), csv_types))
        g.close()
        if rep >= 2:
            for k, v in zip(samples, (ms, ms_cols, ms_floor, ms_csv, ms_csv_cols)):
                samples[k].append(v)
    device = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in samples.items()}
    nbytes = int(d_jsonl.numel())
    for k in ("jsonl_open", "jsonl_columns", "read_floor"):
        device[k]["gb_per_s"] = nbytes / device[k]["median_ms"] / 1e6
    for k in ("csv_open", "csv_columns"):
        device[k]["gb_per_s"] = len(csv_bytes) / device[k]["median_ms"] / 1e6
    # the host form on a prefix of whole lines
    text = d_jsonl.cpu().numpy().tobytes()
    cut = 0
    for _ in range(min(args.host_rows, rows)):
        cut = text.index(b"\n", cut) + 1
    head = text[:cut]
    host = {"rows": min(args.host_rows, rows), "bytes": len(head), "read_jsonl_ms": [], "json_loads_ms": []}
    for rep in range(3):
        t0 = time.perf_counter()
        tabular.read_jsonl(head, ctx=ctx)
        t1 = time.perf_counter()
        for line in head.splitlines():
            json.loads(line)
        t2 = time.perf_counter()
        if rep:
            host["read_jsonl_ms"].append((t1 - t0) * 1e3), host["json_loads_ms"].append((t2 - t1) * 1e3)
    out = {"rows": rows, "jsonl_bytes": nbytes, "csv_bytes": len(csv_bytes), "names": names, "types": [tabular.CSV_TYPE_NAMES[t] for t in jsonl_types],
           "stats8": list(stats), "reps": args.reps, "device": device, "host": host}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
