"""The Parquet writer's list columns (oxh_write_parquet_lists_device) at the size of real tables, columns already in HBM:
  embeddings  --emb-rows (1 M) x 768 float32 fixed-length lists, no nulls: both level streams RLE, the straight copy;
  lists       --list-rows (10 M) rows of list<int64>, lengths 0 to 5, a tenth null lists and a tenth null elements.
Per frame it records, and fixes nothing in advance: the writing call at a capacity measured before (the count, the
levels, the plan coming down, the emit), one `torch` device-to-device copy of the file's bytes (the floor), the flat
writer on one flat 8-byte column of as many values -- alternated in one loop, so they see the same machine -- and
`pyarrow.parquet.write_table` of the same columns from host memory on 16 threads. Two warm calls, medians of --reps, a
host clock around calls that block until the device is done. Then the same call under OXH_TRACE, where the library
times its list steps apart by events (`steps`).

    python tools/parquet_write_lists_probe.py [--emb-rows 1000000] [--list-rows 10000000] [--reps 5] [--out profiles/parquet_write_lists/probe.json]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from csv_probe import timing  # noqa: E402
from json_write_probe import alternated  # noqa: E402


def frames(args):
    rng = np.random.default_rng(5)
    n, dim = args.emb_rows, 768
    yield "embeddings", (rng.standard_normal(n * dim, dtype=np.float32), np.arange(n + 1, dtype=np.int32 if n * dim < 2**31 else np.int64) * dim, None, None)
    n = args.list_rows
    offsets = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(rng.integers(0, 6, n), out=offsets[1:])
    bits = lambda count: np.packbits(rng.random(count) >= 0.1, bitorder="little")  # noqa: E731
    yield "lists", (rng.integers(-(1 << 62), 1 << 62, int(offsets[-1])), offsets, bits(n), bits(int(offsets[-1])))


def steps(call, reps):
    """The call under OXH_TRACE: the library's PQL_STEPS and PQL_FREE lines (events around the list steps, a host clock
    around the allocations, the wait for the totals and the frees), medians over reps calls."""
    import re
    import statistics
    import tempfile

    seen = {}
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.environ["OXH_TRACE"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            for _ in range(reps):
                call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            del os.environ["OXH_TRACE"]
        tmp.seek(0)
        for line in tmp.read().decode(errors="replace").splitlines():
            found = re.match(r"PQL_(STEPS|FREE) (\{.*\})", line)
            if found:
                for key, ms in json.loads(found.group(2)).items():
                    seen.setdefault(key, []).append(ms)
    return {key: round(statistics.median(ms), 3) for key, ms in seen.items()}


def measure(name, parts, reps):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.hasher import default_context

    ctx = default_context()
    up = lambda a: None if a is None else torch.from_numpy(a).to("cuda:0")  # noqa: E731
    values, offsets, validity, child = parts
    frame = {"v": tabular.ListColumn(*(up(a) for a in parts))}
    flat = {"v": tabular.Column(_capi.OXH_COL_FIXED8, values.size * values.itemsize // 8, up(values.view(np.uint8)).view(torch.int64))}
    data, stats = tabular.write_parquet_device(frame, ctx=ctx, stream=ctx.stream, with_stats=True)
    other, flat_bytes = torch.empty_like(data), tabular.write_parquet_device(flat, ctx=ctx, stream=ctx.stream).numel()

    def floor():
        other.copy_(data)
        torch.cuda.synchronize()

    t = alternated({"call": lambda: tabular.write_parquet_device(frame, ctx=ctx, stream=ctx.stream, capacity=stats.bytes),
                    "copy_floor": floor,
                    "flat_writer_same_values": lambda: tabular.write_parquet_device(flat, ctx=ctx, stream=ctx.stream, capacity=flat_bytes)}, reps)
    mask = lambda m, count: None if m is None else ~np.unpackbits(m, bitorder="little")[:count].astype(bool)  # noqa: E731
    elements = pa.array(values, mask=mask(child, values.size))
    make = pa.LargeListArray if offsets.dtype == np.int64 else pa.ListArray
    table = pa.table({"v": make.from_arrays(pa.array(offsets), elements, mask=None if validity is None else pa.array(mask(validity, offsets.size - 1)))})
    pa.set_cpu_count(16)
    t["pyarrow_write_table_16_threads"] = timing(lambda: pq.write_table(table, io.BytesIO(), compression="none", use_dictionary=False), reps)
    rate = lambda ms: round(stats.bytes / 1e9 / (ms / 1e3), 1)  # noqa: E731
    t.update({"file_bytes": stats.bytes, "stats4": list(stats), "rows": offsets.size - 1, "elements": int(values.size),
              "call_gb_s_of_file": rate(t["call"]["median_ms"]), "floor_gb_s_one_way": rate(t["copy_floor"]["median_ms"]),
              "call_over_floor": round(t["call"]["median_ms"] / t["copy_floor"]["median_ms"], 2),
              "call_over_flat_writer": round(t["call"]["median_ms"] / t["flat_writer_same_values"]["median_ms"], 2),
              "steps": steps(lambda: tabular.write_parquet_device(frame, ctx=ctx, stream=ctx.stream, capacity=stats.bytes), reps)})
    print(name, json.dumps(t), flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emb-rows", type=int, default=1_000_000)
    ap.add_argument("--list-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parquet_write_lists", "probe.json"))
    args = ap.parse_args()
    import torch

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    for name, parts in frames(args):
        result[name] = measure(name, parts, args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
