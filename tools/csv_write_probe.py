"""The CSV writer (oxh_write_csv_*) at the size of a real table, on the four files of tools/csv_probe.py: --rows (10 M)
rows of the five-column shape (Int64, Float64, Boolean, two short strings), one wide numeric file (50 Int64 columns),
and two float files of --float-rows rows (at most 15 significant digits; repr() of random doubles). Every frame is
what `read_csv_device` gives for the file's text, so the columns are in HBM as the chain leaves them. It records, and
fixes nothing in advance:
  device   the measuring call (out NULL) and the writing call (into a buffer made before) apart, each beside one
           `torch` device-to-device copy of the output's bytes in the same run as the floor, and the ratio to it;
  floats   the deferred share of both float files, and the cost per deferred cell: the measuring call of the repr()
           file over that of the 15-digit file (the same rows, no cell deferred), divided by the deferred cells;
  host     the host form end to end (`write_csv` from host columns to host bytes) for the five-column file, beside
           `pyarrow.csv.write_csv` and `pandas.DataFrame.to_csv` of the same table on the host in the same run where
           they import ("absent" where they do not).
Two warm calls, medians of --reps, a host clock around calls that block until the device is done. There is no pass /
fail threshold on any of it.

    python tools/csv_write_probe.py [--rows 10000000] [--reps 5] [--out profiles/csv_write/probe.json]
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

from csv_probe import five_columns, float_file, timing, wide_numeric  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--float-rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv_write", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.device import _stream

    if not torch.cuda.is_available():
        sys.exit("csv_write_probe: no GPU (there is nothing to measure on a CPU)")
    ctx = _capi.Context(0)
    rng = np.random.default_rng(a.seed)
    sync = torch.cuda.synchronize
    out = {"rows": a.rows, "reps": a.reps, "files": {}}

    def case_of(data, rows, name, host_too):
        d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        frame = tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream)
        del d
        cols = list(frame.values())
        assert cols[0].nrows == rows
        head = tabular._write_head(frame, ",", '"', True, None)
        cols, type_words, name_bytes, name_offsets, tail = head
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
        tables = tabular._tables(cols, ptr)
        fn = _capi.lib().oxh_write_csv_device
        fixed = (fn, "oxh_write_csv_device", ctx, cols, type_words, tables, name_bytes, name_offsets, tail)
        need, stats = tabular._write_call(*fixed, None, 0, _stream(ctx.stream))
        buf = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        other = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        sync()

        def floor():
            other.copy_(buf)
            sync()

        case = {"rows": rows, "columns": len(cols), "types": [tabular.CSV_TYPE_NAMES[int(t)] for t in type_words][:len(cols)],
                "output_bytes": need, "input_text_bytes": len(data), "stats4": list(stats),
                "measure": timing(lambda: tabular._write_call(*fixed, None, 0, _stream(ctx.stream)), a.reps),
                "write_into_a_buffer": timing(lambda: tabular._write_call(*fixed, buf.data_ptr(), need, _stream(ctx.stream)), a.reps),
                "copy_floor": timing(floor, a.reps)}
        # the writing call measures first: what it adds to the measure is the scan and the emit
        f_ms = case["copy_floor"]["median_ms"]
        case["write_over_floor"] = round(case["write_into_a_buffer"]["median_ms"] / f_ms, 2)
        case["measure_over_floor"] = round(case["measure"]["median_ms"] / f_ms, 2)
        case["write_gb_s"] = round(need / 1e9 / (case["write_into_a_buffer"]["median_ms"] / 1e3), 1)
        case["floor_gb_s_one_way"] = round(need / 1e9 / (f_ms / 1e3), 1)
        nfloat = sum(int(t) == _capi.OXH_CSV_FLOAT64 for t in list(type_words)[:len(cols)]) * rows
        case["float_cells"] = nfloat
        case["deferred_share_of_float_cells"] = round(stats.deferred / nfloat, 4) if nfloat else None
        if host_too:
            host_frame = {n: tabular.Column(c.kind, c.nrows, *(None if x is None else x.cpu().numpy() for x in (c.values, c.offsets, c.validity)))
                          for n, c in frame.items()}
            written = tabular.write_csv(host_frame, ctx=ctx)
            assert written == buf.cpu().numpy().tobytes(), "the two forms differ"
            case["host_form_end_to_end"] = timing(lambda: tabular.write_csv(host_frame, ctx=ctx), a.reps)
            try:
                import pyarrow as pa
                import pyarrow.csv as pacsv

                pa.set_cpu_count(16)
                table = pacsv.read_csv(io.BytesIO(data), parse_options=pacsv.ParseOptions(newlines_in_values=True))

                def arrow_write():
                    sink = io.BytesIO()
                    pacsv.write_csv(table, sink)

                case["pyarrow_write_csv_16_threads"] = timing(arrow_write, a.reps, warm=1)
                try:
                    df = table.to_pandas()
                    case["pandas_to_csv"] = timing(lambda: df.to_csv(io.StringIO(), index=False), 1, warm=0)
                except ImportError:
                    case["pandas_to_csv"] = "absent"
            except ImportError:
                case["pyarrow_write_csv_16_threads"] = "absent"
                case["pandas_to_csv"] = "absent (needs the pyarrow table here)"
        out["files"][name] = case
        print(name, json.dumps(case), flush=True)

    data, rows = five_columns(rng, a.rows)
    case_of(data, rows, "five_columns", host_too=True)
    data, rows = wide_numeric(rng, a.wide_rows)
    case_of(data, rows, "wide_numeric", host_too=False)
    data, rows = float_file(rng, a.float_rows, short=True)
    case_of(data, rows, "floats_15_digits", host_too=False)
    data, rows = float_file(rng, a.float_rows, short=False)
    case_of(data, rows, "floats_repr", host_too=False)
    short, long_ = out["files"]["floats_15_digits"], out["files"]["floats_repr"]
    deferred = long_["stats4"][2]
    out["deferral"] = {"share_15_digits": short["deferred_share_of_float_cells"], "share_repr": long_["deferred_share_of_float_cells"],
                       "measure_ms_15_digits": short["measure"]["median_ms"], "measure_ms_repr": long_["measure"]["median_ms"],
                       "write_ms_15_digits": short["write_into_a_buffer"]["median_ms"], "write_ms_repr": long_["write_into_a_buffer"]["median_ms"],
                       "deferred_cells_repr": deferred,
                       "ns_per_deferred_cell": round((long_["measure"]["median_ms"] - short["measure"]["median_ms"]) * 1e6 / deferred, 1) if deferred else None}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
