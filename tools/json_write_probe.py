"""The JSON writer (oxh_write_json_*) at the size of a real table. Every frame is what `read_csv_device` gives for a
file's text, so the columns are in HBM as the chain leaves them. It records, and fixes nothing in advance:
  (a) tables  --rows (10 M) rows of tools/csv_probe.py's five-column shape (Int64, Float64, Boolean, two short
              strings) and --wide-rows (1 M) rows of 50 Int64 columns, in both formats: the measuring call (out NULL)
              and the writing call (into a buffer made before), beside one `torch` device-to-device copy of the
              output's bytes and `oxh_write_csv_device` of the same frame -- all alternated in one loop, so the pairs
              see the same machine. The JSON text is larger (every row carries its keys): compare GB/s of output;
  (b) long    --long-rows (100 000) rows with one string cell of about 4 KiB, once with no byte to escape (the whole
              wave copies the cell), once with a '\\n' about every 60 bytes (the whole wave escapes it, 64 source
              bytes a step): both rates and their ratio price the escaping path;
  (c) host    the host form end to end (`write_jsonl` from host columns to host bytes) on --host-rows (1 M) rows of
              the five-column shape, beside `json.dumps` per row and `pandas.DataFrame.to_json(orient="records",
              lines=True)` of the same rows in the same run where pandas imports ("absent" where it does not).
Two warm calls, medians of --reps, a host clock around calls that block until the device is done. There is no pass /
fail threshold on any of it.

    python tools/json_write_probe.py [--rows 10000000] [--reps 5] [--out profiles/json_write/probe.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from csv_probe import five_columns, timing, wide_numeric  # noqa: E402


def alternated(calls: dict, reps: int, warm: int = 2) -> dict:
    """Every call once per round, round after round: {name: timing}. A pair's spread is the rounds' own."""
    for _ in range(warm):
        for call in calls.values():
            call()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "reps": reps}
            for name, t in times.items()}


def long_cells(rows: int, escaped: bool):
    """rows records of (Int64, one quoted string cell of 4096 bytes); escaped: a '\\n' as every 60th byte."""
    line = ("the quick brown fox jumps over the lazy dog, again and again " * 2)[:59]
    cell = ((line + ("\n" if escaped else " ")) * 70)[:4096]
    n = min(rows, 1000)
    block = "".join('%d,"%s"\n' % (k, cell) for k in range(n))
    return ("k,text\n" + block * (rows // n)).encode(), (rows // n) * n, cell.count("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--long-rows", type=int, default=100_000)
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_write", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.device import _stream

    if not torch.cuda.is_available():
        sys.exit("json_write_probe: no GPU (there is nothing to measure on a CPU)")
    ctx = _capi.Context(0)
    rng = np.random.default_rng(a.seed)
    sync = torch.cuda.synchronize
    out = {"rows": a.rows, "reps": a.reps, "tables": {}, "long_cells": {}, "host": {}}
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    stream = _stream(ctx.stream)
    FORMATS = (("jsonl", _capi.OXH_JSON_LINES), ("json", _capi.OXH_JSON_ARRAY))

    def frame_of(data, rows):
        d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        frame = tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream)
        del d
        assert next(iter(frame.values())).nrows == rows
        return frame

    def json_call(frame, flags):
        cols, type_words, name_bytes, name_offsets, tail = tabular._json_head(frame, None, flags)
        tables = tabular._tables(cols, ptr)
        return (_capi.lib().oxh_write_json_device, "oxh_write_json_device", ctx, cols, type_words, tables, name_bytes, name_offsets, tail)

    def csv_call(frame):
        cols, type_words, name_bytes, name_offsets, tail = tabular._write_head(frame, ",", '"', True, None)
        tables = tabular._tables(cols, ptr)
        return (_capi.lib().oxh_write_csv_device, "oxh_write_csv_device", ctx, cols, type_words, tables, name_bytes, name_offsets, tail)

    def rate(nbytes, ms):
        return round(nbytes / 1e9 / (ms / 1e3), 1)

    def table_case(data, rows, name):
        frame = frame_of(data, rows)
        fixed_csv = csv_call(frame)
        csv_need, _ = tabular._write_call(*fixed_csv, None, 0, stream)
        csv_buf = torch.empty(csv_need, dtype=torch.uint8, device="cuda:0")
        case = {"rows": rows, "columns": len(frame), "input_text_bytes": len(data), "csv_output_bytes": csv_need}
        for label, flags in FORMATS:
            fixed = json_call(frame, flags)
            need, stats = tabular._write_call(*fixed, None, 0, stream)
            buf = torch.empty(need, dtype=torch.uint8, device="cuda:0")
            other = torch.empty(need, dtype=torch.uint8, device="cuda:0")
            sync()

            def floor():
                other.copy_(buf)
                sync()

            t = alternated({"measure": lambda: tabular._write_call(*fixed, None, 0, stream),
                            "write_into_a_buffer": lambda: tabular._write_call(*fixed, buf.data_ptr(), need, stream),
                            "csv_write_into_a_buffer": lambda: tabular._write_call(*fixed_csv, csv_buf.data_ptr(), csv_need, stream),
                            "copy_floor": floor}, a.reps)
            t.update({"output_bytes": need, "stats4": list(stats),
                      "write_gb_s": rate(need, t["write_into_a_buffer"]["median_ms"]),
                      "write_gb_s_min_max": [rate(need, t["write_into_a_buffer"]["max_ms"]), rate(need, t["write_into_a_buffer"]["min_ms"])],
                      "csv_write_gb_s": rate(csv_need, t["csv_write_into_a_buffer"]["median_ms"]),
                      "csv_write_gb_s_min_max": [rate(csv_need, t["csv_write_into_a_buffer"]["max_ms"]), rate(csv_need, t["csv_write_into_a_buffer"]["min_ms"])],
                      "floor_gb_s_one_way": rate(need, t["copy_floor"]["median_ms"]),
                      "write_over_floor": round(t["write_into_a_buffer"]["median_ms"] / t["copy_floor"]["median_ms"], 2)})
            case[label] = t
            del buf, other
        out["tables"][name] = case
        print(name, json.dumps(case), flush=True)

    data, rows = five_columns(rng, a.rows)
    table_case(data, rows, "five_columns")
    data, rows = wide_numeric(rng, a.wide_rows)
    table_case(data, rows, "wide_numeric")

    # (b) the long cells: the same rows, plain and with a '\n' about every 60 bytes
    for name, escaped in (("plain", False), ("escaped", True)):
        data, rows, per_cell = long_cells(a.long_rows, escaped)
        frame = frame_of(data, rows)
        fixed = json_call(frame, _capi.OXH_JSON_LINES)
        need, stats = tabular._write_call(*fixed, None, 0, stream)
        buf = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        sync()
        t = alternated({"measure": lambda: tabular._write_call(*fixed, None, 0, stream),
                        "write_into_a_buffer": lambda: tabular._write_call(*fixed, buf.data_ptr(), need, stream)}, a.reps)
        t.update({"rows": rows, "cell_bytes": 4096, "escapes_per_cell": per_cell, "output_bytes": need, "stats4": list(stats),
                  "write_gb_s": rate(need, t["write_into_a_buffer"]["median_ms"]), "measure_gb_s": rate(need, t["measure"]["median_ms"]),
                  # the writing call measures first: what it adds is the scan and the emit
                  "emit_gb_s": rate(need, max(t["write_into_a_buffer"]["median_ms"] - t["measure"]["median_ms"], 1e-3))})
        out["long_cells"][name] = t
        print(name, json.dumps(t), flush=True)
        del buf, frame
    plain, esc = out["long_cells"]["plain"], out["long_cells"]["escaped"]
    out["long_cells"]["plain_over_escaped_write_rate"] = round(plain["write_gb_s"] / esc["write_gb_s"], 2)
    out["long_cells"]["plain_over_escaped_emit_rate"] = round(plain["emit_gb_s"] / esc["emit_gb_s"], 2)

    # (c) the host form end to end, beside the host's own writers
    data, rows = five_columns(rng, a.host_rows)
    frame = frame_of(data, rows)
    host_frame = {n: tabular.Column(c.kind, c.nrows, *(None if x is None else x.cpu().numpy() for x in (c.values, c.offsets, c.validity)))
                  for n, c in frame.items()}
    written = tabular.write_jsonl(host_frame, ctx=ctx)
    assert written == tabular.write_jsonl_device(frame, ctx=ctx).cpu().numpy().tobytes(), "the two forms differ"
    host = {"rows": rows, "output_bytes": len(written), "host_form_end_to_end": timing(lambda: tabular.write_jsonl(host_frame, ctx=ctx), a.reps)}
    records = [json.loads(line) for line in written.decode().splitlines()]

    def dumps_per_row():
        return "".join(json.dumps(r, separators=(",", ":")) + "\n" for r in records)

    host["json_dumps_per_row"] = timing(dumps_per_row, max(1, min(a.reps, 3)), warm=0)
    try:
        import pandas as pd

        df = pd.DataFrame.from_records(records)
        host["pandas_to_json_records_lines"] = timing(lambda: df.to_json(orient="records", lines=True), max(1, min(a.reps, 3)), warm=0)
    except ImportError:
        host["pandas_to_json_records_lines"] = "absent"
    out["host"] = host
    print("host", json.dumps(host), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
