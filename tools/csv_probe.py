"""The CSV reader (oxh_csv_*) at the size of a real table: --rows (10 M) rows of the five-column shape the other
probes use (Int64, Float64, Boolean, two short strings), one wide numeric file (50 columns), and two float files of
--float-rows rows (at most 15 significant digits; repr() of random doubles). It records, and fixes nothing in advance:
  device   the bytes already in HBM: the open (the index) and the columns (measure, output allocation and write, as
           `CsvFile.columns` does them), each beside a plain device read of the same bytes in the same run
           (`torch.sum` over the buffer) as the floor, and the ratio to it;
  host     the host form end to end (open + columns from host bytes), beside `pyarrow.csv.read_csv` with 16 threads
           and `pandas.read_csv` on the same bytes in the same run where they import ("absent" where they do not);
  floats   the deferred share of both float files and the time of their column;
  memory   bytes of working memory per input byte, COMPUTED from the file's counts by the sizes csv_host.hpp states
           (36 B per 4 KiB tile, 4 B per delimiter and 8 B per record, 20 B per 64 records, 12 B per row under a
           string column, 12 B per 64 rows per Float64 column and 8 B per 64 rows once, 68 B per deferred cell on
           the device and as much on the host) -- not read from the library: the 256-byte rounding of every array
           and the scans' tile sums (8 B per 2 048 entries) are left out.
Two warm calls, medians of --reps, a host clock around calls that block until the device is done. Every file is
built from a block of 100 000 generated rows repeated: the parser's work does not depend on the repetition.

    python tools/csv_probe.py [--rows 10000000] [--reps 5] [--out profiles/csv/probe.json]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 100_000


def five_columns(rng, rows):
    n = min(rows, BLOCK)
    ints = rng.integers(-2**40, 2**40, size=n).tolist()
    floats = (rng.integers(-2**16, 2**16, size=n) / 1024.0).tolist()
    flags = (rng.random(n) < 0.5).tolist()
    a = rng.integers(0, 100, size=n).tolist()
    b = rng.integers(0, 10**9, size=n).tolist()
    block = "".join("%d,%r,%s,label-%03d,\"id %d, x\"\n" % (i, f, "true" if t else "false", x, y) for i, f, t, x, y in zip(ints, floats, flags, a, b))
    return ("i,f,b,label,note\n" + block * (rows // n)).encode(), (rows // n) * n


def wide_numeric(rng, rows, width=50):
    n = min(rows, BLOCK // 10)
    values = rng.integers(-10**6, 10**6, size=(n, width))
    block = "\n".join(",".join(map(str, row)) for row in values.tolist()) + "\n"
    return (",".join("c%d" % k for k in range(width)) + "\n" + block * (rows // n)).encode(), (rows // n) * n


def float_file(rng, rows, short):
    n = min(rows, BLOCK)
    if short:
        cells = [repr(v) for v in (rng.integers(-2**20, 2**20, size=n) / 1024.0).tolist()]
    else:
        cells = [repr(v) for v in rng.standard_normal(n).tolist()]
    return ("x\n" + ("\n".join(cells) + "\n") * (rows // n)).encode(), (rows // n) * n


def median_ms(call, reps, warm=2):
    for _ in range(warm):
        call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def timing(call, reps, warm=2):
    med, lo, hi = median_ms(call, reps, warm)
    return {"median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--float-rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular

    if not torch.cuda.is_available():
        sys.exit("csv_probe: no GPU (there is nothing to measure on a CPU)")
    ctx = _capi.Context(0)
    rng = np.random.default_rng(a.seed)
    sync = torch.cuda.synchronize
    out = {"rows": a.rows, "reps": a.reps, "files": {}}

    def device_case(data, rows, name, host_too):
        d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        sync()
        gb = len(data) / 1e9

        def floor():
            d.sum(dtype=torch.int64)
            sync()

        case = {"bytes": len(data), "rows": rows, "read_floor": timing(floor, a.reps)}
        with tabular.CsvFile(d, ctx=ctx, device=True, stream=ctx.stream) as f:
            types = f.infer()
            cols = list(range(f.stats.ncols))
            assert f.stats.rows == rows, (f.stats, rows)
            case["stats8"] = list(f.stats)
            case["types"] = [tabular.CSV_TYPE_NAMES[t] for t in types]
            case["infer_10000_rows"] = timing(lambda: f.infer(), a.reps)
            case["columns"] = timing(lambda: f.columns(cols, types), a.reps)
            _, stats = f.columns(cols, types, with_stats=True)
            case["deferred_cells"] = sum(s.deferred for s in stats)
            s = f.stats
            tiles = -(-(len(data) + 1) // 4096)
            nstrings = sum(t in (_capi.OXH_CSV_STRING, _capi.OXH_CSV_STRING64) for t in types)
            nfloats = sum(t == _capi.OXH_CSV_FLOAT64 for t in types)
            case["computed_working_bytes_per_input_byte"] = {
                "index_lease": round(36 * tiles / len(data), 5),
                "handle_arrays": round((4 * s.delimiters + 8 * s.records) / len(data), 5),
                "row_map_lease": round(20 * -(-s.records // 64) / len(data), 5),
                "columns_lease": round(((12 * s.rows if nstrings else 0) + nfloats * 12 * -(-s.rows // 64) + 8 * -(-s.rows // 64)) / len(data), 5),
                "deferred_block": round(68 * case["deferred_cells"] / len(data), 5),
            }

        def open_close():
            tabular.CsvFile(d, ctx=ctx, device=True, stream=ctx.stream).close()

        case["open"] = timing(open_close, a.reps)
        f_ms = case["read_floor"]["median_ms"]
        case["open_over_floor"] = round(case["open"]["median_ms"] / f_ms, 2)
        case["columns_over_floor"] = round(case["columns"]["median_ms"] / f_ms, 2)
        case["open_gb_s"] = round(gb / (case["open"]["median_ms"] / 1e3), 1)
        case["columns_gb_s"] = round(gb / (case["columns"]["median_ms"] / 1e3), 1)
        case["floor_gb_s"] = round(gb / (f_ms / 1e3), 1)
        if host_too:
            host = np.frombuffer(data, dtype=np.uint8)

            def host_form():
                with tabular.CsvFile(host, ctx=ctx) as g:
                    g.columns(cols, types)

            case["host_form_end_to_end"] = timing(host_form, a.reps)
            try:
                import pyarrow as pa
                import pyarrow.csv as pacsv

                pa.set_cpu_count(16)
                case["pyarrow_16_threads"] = timing(lambda: pacsv.read_csv(io.BytesIO(data), read_options=pacsv.ReadOptions(use_threads=True),
                                                                           parse_options=pacsv.ParseOptions(newlines_in_values=True)), a.reps, warm=1)
            except ImportError:
                case["pyarrow_16_threads"] = "absent"
            try:
                import pandas as pd

                case["pandas"] = timing(lambda: pd.read_csv(io.BytesIO(data)), max(1, a.reps // 3), warm=1)
            except ImportError:
                case["pandas"] = "absent"
        out["files"][name] = case
        print(name, json.dumps(case), flush=True)
        del d

    data, rows = five_columns(rng, a.rows)
    device_case(data, rows, "five_columns", host_too=True)
    data, rows = wide_numeric(rng, a.wide_rows)
    device_case(data, rows, "wide_numeric", host_too=False)
    data, rows = float_file(rng, a.float_rows, short=True)
    device_case(data, rows, "floats_15_digits", host_too=False)
    data, rows = float_file(rng, a.float_rows, short=False)
    device_case(data, rows, "floats_repr", host_too=False)
    short, long_ = out["files"]["floats_15_digits"], out["files"]["floats_repr"]
    out["deferral"] = {"share_15_digits": round(short["deferred_cells"] / short["rows"], 4), "share_repr": round(long_["deferred_cells"] / long_["rows"], 4),
                       "columns_ms_15_digits": short["columns"]["median_ms"], "columns_ms_repr": long_["columns"]["median_ms"],
                       "bytes_15_digits": short["bytes"], "bytes_repr": long_["bytes"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
