"""The Parquet reader (oxh_parquet_*) at the size of a real table: --rows (10 M) rows of tools/csv_probe.py's
five-column shape (Int64, Float64, Boolean, two short strings), as `write_parquet_device` leaves the file in HBM (PLAIN
values, DataPage V1) and, where pyarrow imports, the same table from pyarrow with dictionaries on and compression off.
Per file it records, and fixes nothing in advance:
  (a) device  the open (footer and page walk), the measure of the string columns that `ParquetFile.columns` makes
              before it allocates, the fill into buffers made before, and the strings' fill alone, beside one `torch`
              device-to-device copy of the file's bytes (the floor) -- all alternated in one loop, so they see the same
              machine; and `read_parquet_device` whole (open, measure, allocate, fill);
  (b) host    `pyarrow.parquet.read_table` of the same bytes in host memory with 16 threads, and `read_parquet` from
              host bytes to host columns ("absent" where pyarrow does not import).
Two warm calls, medians of --reps, a host clock around calls that block until the device is done. There is no pass /
fail threshold on any of it.

    python tools/parquet_read_probe.py [--rows 10000000] [--reps 5] [--out profiles/parquet_read/probe.json]
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

from csv_probe import five_columns, timing  # noqa: E402
from json_write_probe import alternated  # noqa: E402


def device_times(tabular, _capi, torch, ctx, d_file, reps):
    """The device calls over one file's bytes on the device."""
    sync = torch.cuda.synchronize
    other = torch.empty_like(d_file)
    rate = lambda nbytes, ms: round(nbytes / 1e9 / (ms / 1e3), 1)  # noqa: E731
    with tabular.ParquetFile(d_file, ctx=ctx, device=True, stream=ctx.stream) as f:
        types = [t.type for t in f.types()]
        picked = list(range(len(types)))
        strings = [k for k in picked if types[k] in (_capi.OXH_CSV_STRING, _capi.OXH_CSV_STRING64)]
        cols, stats = f.columns(picked, types, with_stats=True)   # the buffers the fill goes into, made before
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731

        def tables(which):
            m = max(len(which), 1)
            return [(ctypes.c_void_p * m)(*[ptr(getattr(cols[k], field)) for k in which]) for field in ("values", "offsets", "validity")]

        def fill(which):
            _, _, col_idx, type_words = f._selection(which, [types[k] for k in which])
            capacity = np.array([cols[k].values.numel() * cols[k].values.element_size() for k in which], dtype=np.uint64)
            return lambda: f._call(len(which), col_idx, type_words, capacity, *tables(which))

        def opened():
            tabular.ParquetFile(d_file, ctx=ctx, device=True, stream=ctx.stream).close()

        def floor():
            other.copy_(d_file)
            sync()

        t = alternated({"open": opened, "measure_strings": lambda: f.measure(strings, [types[k] for k in strings]), "fill_into_buffers": fill(picked),
                        "fill_strings_only": fill(strings), "read_parquet_device_whole": lambda: tabular.read_parquet_device(d_file, ctx=ctx, stream=ctx.stream),
                        "copy_floor": floor}, reps)
        out_bytes = sum(sum(x.numel() * x.element_size() for x in (c.values, c.offsets, c.validity) if x is not None) for c in cols)
        t.update({"file_bytes": d_file.numel(), "column_bytes": out_bytes, "stats8": list(f.stats), "stats4": [list(s) for s in stats],
                  "fill_gb_s_of_file": rate(d_file.numel(), t["fill_into_buffers"]["median_ms"]),
                  "floor_gb_s_one_way": rate(d_file.numel(), t["copy_floor"]["median_ms"]),
                  "fill_over_floor": round(t["fill_into_buffers"]["median_ms"] / t["copy_floor"]["median_ms"], 2),
                  "strings_share_of_fill": round(t["fill_strings_only"]["median_ms"] / t["fill_into_buffers"]["median_ms"], 2)})
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parquet_read", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular

    if not torch.cuda.is_available():
        sys.exit("parquet_read_probe: no GPU (there is nothing to measure on a CPU)")
    ctx = _capi.Context(0)
    data, rows = five_columns(np.random.default_rng(a.seed), a.rows)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    frame = tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream)
    del d
    d_ours = tabular.write_parquet_device(frame, ctx=ctx, stream=ctx.stream)
    del frame
    out = {"rows": rows, "reps": a.reps, "our_file": {"device": device_times(tabular, _capi, torch, ctx, d_ours, a.reps)}}
    print(json.dumps(out["our_file"]), flush=True)
    ours = d_ours.cpu().numpy().tobytes()
    out["our_file"]["host"] = {"read_parquet": timing(lambda: tabular.read_parquet(ours, ctx=ctx), a.reps)}
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq

        pa.set_cpu_count(16)
        out["our_file"]["host"]["pyarrow_read_table_16_threads"] = timing(lambda: pq.read_table(io.BytesIO(ours)), a.reps)
        sink = io.BytesIO()
        pq.write_table(pq.read_table(io.BytesIO(ours)), sink, compression="none", use_dictionary=True)
        theirs = sink.getvalue()
        d_theirs = torch.from_numpy(np.frombuffer(theirs, dtype=np.uint8).copy()).to("cuda:0")
        out["pyarrow_dictionary_file"] = {"device": device_times(tabular, _capi, torch, ctx, d_theirs, a.reps),
                                          "host": {"read_parquet": timing(lambda: tabular.read_parquet(theirs, ctx=ctx), a.reps),
                                                   "pyarrow_read_table_16_threads": timing(lambda: pq.read_table(io.BytesIO(theirs)), a.reps)}}
    except ImportError:
        out["pyarrow_dictionary_file"] = "absent"
    print(json.dumps({k: v for k, v in out.items() if k != "our_file"}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
