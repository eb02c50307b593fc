"""The Parquet reader's list columns (oxh_parquet_lists_*) at the size of real tables, uncompressed and already in HBM:
  embeddings  --emb-rows (1 M) x 768 float32 as fixed_size_list (max definition level 1, no nulls);
  lists       --list-rows (10 M) rows of list<int64>, lengths 0 to 5, null lists and null elements;
  flat        one flat float32 column of as many values as `embeddings` has elements, through oxh_parquet_columns_*.
Per file it records, and fixes nothing in advance: the open, the measure (the level pass, the scans and the totals
coming down), the fill into buffers made before (the measure's work again, then the row and element passes), one
`torch` device-to-device copy of the file's bytes (the floor) -- alternated in one loop, so they see the same machine --
and `pyarrow.parquet.read_table` of the same bytes in host memory on 16 threads. Two warm calls, medians of --reps, a
host clock around calls that block until the device is done.

    python tools/parquet_lists_probe.py [--emb-rows 1000000] [--list-rows 10000000] [--reps 5] [--out profiles/parquet_lists/probe.json]
"""
from __future__ import annotations

import argparse
import ctypes
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


def device_times(tabular, torch, ctx, d_file, reps, lists: bool):
    other = torch.empty_like(d_file)
    rate = lambda nbytes, ms: round(nbytes / 1e9 / (ms / 1e3), 1)  # noqa: E731
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    with tabular.ParquetFile(d_file, ctx=ctx, device=True, stream=ctx.stream) as f:
        types = [f.types()[0].type]
        _, _, col_idx, type_words = f._selection([0], types)
        if lists:
            cols, stats = f.lists([0], types, with_stats=True)   # the buffers the fill goes into, made before
            fields, call = ("values", "offsets", "validity", "child_validity"), f._lists_call
        else:
            cols, stats = f.columns([0], types, with_stats=True)
            fields, call = ("values", "offsets", "validity"), f._call
        tables = [(ctypes.c_void_p * 1)(ptr(getattr(cols[0], field))) for field in fields]
        capacity = np.array([cols[0].values.numel() * cols[0].values.element_size()], dtype=np.uint64)

        def floor():
            other.copy_(d_file)
            torch.cuda.synchronize()

        t = alternated({"open": lambda: tabular.ParquetFile(d_file, ctx=ctx, device=True, stream=ctx.stream).close(),
                        "measure": lambda: call(1, col_idx, type_words, None, *[None] * len(fields)),
                        "fill_into_buffers": lambda: call(1, col_idx, type_words, capacity, *tables), "copy_floor": floor}, reps)
        t.update({"file_bytes": d_file.numel(), "stats8": list(f.stats), "stats4": [list(s) for s in stats],
                  "fill_gb_s_of_file": rate(d_file.numel(), t["fill_into_buffers"]["median_ms"]),
                  "floor_gb_s_one_way": rate(d_file.numel(), t["copy_floor"]["median_ms"]),
                  "fill_over_floor": round(t["fill_into_buffers"]["median_ms"] / t["copy_floor"]["median_ms"], 2),
                  "rows_and_elements_ms": round(t["fill_into_buffers"]["median_ms"] - t["measure"]["median_ms"], 3)})
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emb-rows", type=int, default=1_000_000)
    ap.add_argument("--list-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parquet_lists", "probe.json"))
    a = ap.parse_args()

    import pyarrow as pa
    import pyarrow.parquet as pq
    import torch

    from oxen_amd import _capi, tabular

    if not torch.cuda.is_available():
        sys.exit("parquet_lists_probe: no GPU (there is nothing to measure on a CPU)")
    pa.set_cpu_count(16)
    ctx = _capi.Context(0)
    rng = np.random.default_rng(a.seed)
    dim = 768
    flat = pa.array(rng.random(a.emb_rows * dim, dtype=np.float32))
    lengths = rng.integers(0, 6, a.list_rows)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    elements = pa.array(rng.integers(-1 << 62, 1 << 62, int(offsets[-1])), mask=rng.random(int(offsets[-1])) < 0.1)
    tables = {"embeddings": (True, pa.table({"e": pa.FixedSizeListArray.from_arrays(flat, dim)})),
              "lists": (True, pa.table({"v": pa.ListArray.from_arrays(pa.array(offsets), elements, mask=pa.array(rng.random(a.list_rows) < 0.1))})),
              "flat": (False, pa.table({"x": flat}))}
    out = {"emb_rows": a.emb_rows, "list_rows": a.list_rows, "reps": a.reps}
    for name in list(tables):
        lists, table = tables.pop(name)
        sink = io.BytesIO()
        pq.write_table(table, sink, compression="none", use_dictionary=False)
        del table
        data = sink.getvalue()
        del sink
        d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        out[name] = {"device": device_times(tabular, torch, ctx, d_file, a.reps, lists),
                     "host": {"pyarrow_read_table_16_threads": timing(lambda: pq.read_table(io.BytesIO(data)), a.reps)}}
        del d_file, data
        torch.cuda.empty_cache()
        print(json.dumps({name: out[name]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
