"""The Parquet writer (oxh_write_parquet_*) at the size of a real table: --rows (10 M) rows of tools/csv_probe.py's
five-column shape (Int64, Float64, Boolean, two short strings), as `read_csv_device` leaves them in HBM. It records,
and fixes nothing in advance:
  (a) device  the measuring call (out NULL) and the writing call (into a buffer made before), beside one `torch`
              device-to-device copy of the output's bytes (the floor) and `oxh_write_csv_device` of the same frame --
              all alternated in one loop, so they see the same machine;
  (b) host    the host form end to end (`write_parquet` from host columns to host bytes) beside
              `pyarrow.parquet.write_table` of the same columns with compression none, no dictionary, 16 threads
              ("absent" where pyarrow does not import); the file the host form wrote is read back by pyarrow and
              compared with its own table.
Two warm calls, medians of --reps, a host clock around calls that block until the device is done. There is no pass /
fail threshold on any of it.

    python tools/parquet_write_probe.py [--rows 10000000] [--reps 5] [--out profiles/parquet_write/probe.json]
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

from csv_probe import five_columns, timing  # noqa: E402
from json_write_probe import alternated  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parquet_write", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.device import _stream
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("parquet_write_probe: no GPU (there is nothing to measure on a CPU)")
    ctx = _capi.Context(0)
    sync = torch.cuda.synchronize
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    stream = _stream(ctx.stream)
    rate = lambda nbytes, ms: round(nbytes / 1e9 / (ms / 1e3), 1)  # noqa: E731

    data, rows = five_columns(np.random.default_rng(a.seed), a.rows)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    frame = tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream)
    del d
    cols, type_words, name_bytes, name_offsets, tail = tabular._parquet_head(frame, None, None, None)
    fixed = (_capi.lib().oxh_write_parquet_device, "oxh_write_parquet_device", ctx, cols, type_words, tabular._tables(cols, ptr), name_bytes, name_offsets, tail)
    ccols, ctypes_, cnames, coffs, ctail = tabular._write_head(frame, ",", '"', True, None)
    fixed_csv = (_capi.lib().oxh_write_csv_device, "oxh_write_csv_device", ctx, ccols, ctypes_, tabular._tables(ccols, ptr), cnames, coffs, ctail)
    need, stats = tabular._write_call(*fixed, None, 0, stream)
    csv_need, _ = tabular._write_call(*fixed_csv, None, 0, stream)
    buf, other = (torch.empty(need, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    csv_buf = torch.empty(csv_need, dtype=torch.uint8, device="cuda:0")
    sync()

    def floor():
        other.copy_(buf)
        sync()

    t = alternated({"measure": lambda: tabular._write_call(*fixed, None, 0, stream),
                    "write_into_a_buffer": lambda: tabular._write_call(*fixed, buf.data_ptr(), need, stream),
                    "csv_write_into_a_buffer": lambda: tabular._write_call(*fixed_csv, csv_buf.data_ptr(), csv_need, stream),
                    "copy_floor": floor}, a.reps)
    t.update({"output_bytes": need, "stats4": [int(x) for x in stats], "csv_output_bytes": csv_need,
              "write_gb_s": rate(need, t["write_into_a_buffer"]["median_ms"]), "csv_write_gb_s": rate(csv_need, t["csv_write_into_a_buffer"]["median_ms"]),
              "floor_gb_s_one_way": rate(need, t["copy_floor"]["median_ms"]),
              "write_over_floor": round(t["write_into_a_buffer"]["median_ms"] / t["copy_floor"]["median_ms"], 2)})
    out = {"rows": rows, "columns": len(frame), "reps": a.reps, "input_text_bytes": len(data), "device": t}
    print(json.dumps({"device": t}), flush=True)

    host_frame = {n: Column(c.kind, c.nrows, *(None if x is None else x.cpu().numpy() for x in (c.values, c.offsets, c.validity)), c.value_bit, c.validity_bit)
                  for n, c in frame.items()}
    written = []

    def ours():
        written[:] = [tabular.write_parquet(host_frame, ctx=ctx)]

    h = {"write_parquet": timing(ours, a.reps)}
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq

        pa.set_cpu_count(16)
        arrays = []
        for c in host_frame.values():
            valid = None if c.validity is None else pa.py_buffer(c.validity)
            if c.kind == _capi.OXH_COL_BOOL:
                arrays.append(pa.Array.from_buffers(pa.bool_(), c.nrows, [valid, pa.py_buffer(c.values)]))
            elif c.kind == _capi.OXH_COL_FIXED8:
                arrays.append(pa.Array.from_buffers(pa.int64() if c.values.dtype == np.int64 else pa.float64(), c.nrows, [valid, pa.py_buffer(c.values)]))
            else:
                arrays.append(pa.Array.from_buffers(pa.string() if c.offsets.dtype == np.int32 else pa.large_string(), c.nrows,
                                                    [valid, pa.py_buffer(c.offsets), pa.py_buffer(c.values)]))
        table = pa.table(arrays, names=list(host_frame))
        sink = []

        def arrow():
            s = io.BytesIO()
            pq.write_table(table, s, compression="none", use_dictionary=False, data_page_version="1.0")
            sink[:] = [s.getbuffer().nbytes]

        h["pyarrow_write_table_16_threads"] = timing(arrow, a.reps)
        h["pyarrow_output_bytes"] = sink[0]
        h["pyarrow_reads_our_file_equal"] = bool(pq.read_table(io.BytesIO(written[-1])).equals(table))
        h["host_over_pyarrow"] = round(h["write_parquet"]["median_ms"] / h["pyarrow_write_table_16_threads"]["median_ms"], 2)
    except ImportError:
        h["pyarrow_write_table_16_threads"] = "absent"
    out["host"] = h
    print(json.dumps({"host": h}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
