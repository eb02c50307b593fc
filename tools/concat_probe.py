"""The concat (oxh_concat_columns_device) at the size of a real table: --rows (10 M) rows of the other probes'
five-column frame (Int64, Float64, Boolean, two strings of 0-48 B):
  parts1 / parts4 / parts64   the whole frame as 1, 4 and 64 row ranges of it, written one after the other;
  head100 / tail100           the first and the last 100 rows: a page of a data-frame view;
  int64 / bool / string       parts1 over one column of that kind alone.
Beside every case, in the same run and alternating with it:
  take    (a) `take_device` with the equivalent `arange` indices -- the only way before this call existed;
  torch   (b) `torch.cat` of the same slices of the fixed-width columns and one `Tensor.copy_` of the byte total of
          each string column -- the plain copies a caller with torch at hand writes (no bitmaps, no offsets).
Both ratios go into the JSON; none is fixed in advance. All inputs device-resident, HIP events on the call's
stream around the blocking call (and the host clock), two warm calls, medians of --reps. Every case is checked:
the concat's columns equal the take's, buffer for buffer (the sources have no nulls, so the two layouts agree).
Which launch takes the time is a matter for `rocprofv3 --kernel-trace --stats -- python tools/concat_probe.py
--reps 3`, in a run of its own.

    python tools/concat_probe.py [--rows 10000000] [--reps 9] [--out profiles/concat/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--cases", default="parts1,parts4,parts64,head100,tail100,int64,bool,string")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concat", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("concat_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    ctx = _capi.Context(0)
    stream = torch.cuda.Stream()
    torch.manual_seed(a.seed)
    n = a.rows

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record(stream)
        with torch.cuda.stream(stream):
            out = fn()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3, out

    def stats(xs):
        ev = [x[0] for x in xs]
        return {"event_ms_median": round(float(np.median(ev)), 4), "event_ms_min": round(min(ev), 4), "event_ms_max": round(max(ev), 4),
                "call_ms_median": round(float(np.median([x[1] for x in xs])), 4)}

    def need(cond, what):
        if not cond:
            sys.exit(f"concat_probe: {what}")

    def strings(m, top):
        lens = torch.randint(0, top + 1, (m,), dtype=torch.int64, device=dev)
        offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        values = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device=dev)
        return Column(tabular.OXH_COL_BYTES32, m, values, offsets.to(torch.int32))

    frame = [Column(8, n, torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev)),
             Column(8, n, torch.randn(n, dtype=torch.float64, device=dev)),
             Column(tabular.OXH_COL_BOOL, n, torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev)),
             strings(n, 48), strings(n, 48)]
    torch.cuda.synchronize()
    result = {"rows": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "cases": {}}

    def same(x, y):
        for c, (p, q) in enumerate(zip(x, y)):
            for name in ("values", "offsets", "validity"):
                s, t = getattr(p, name), getattr(q, name)
                need((s is None) == (t is None) and (s is None or torch.equal(s.view(torch.uint8), t.view(torch.uint8))), f"column {c}: {name} differ")

    def run_case(name, cols, ranges):
        count = sum(c for _, c in ranges)
        idx = torch.cat([torch.arange(f, f + c, dtype=torch.int32, device=dev) for f, c in ranges])
        spans = [[(int(col.offsets[f]), int(col.offsets[f + c])) for f, c in ranges] if col.offsets is not None else None for col in cols]
        room = [torch.empty(sum(hi - lo for lo, hi in s), dtype=torch.uint8, device=dev) if s is not None else None for s in spans]

        def concat():
            return tabular.concat_device([cols] * len(ranges), ranges, stream=stream.cuda_stream, ctx=ctx)

        def take():
            return tabular.take_device(cols, idx, stream=stream.cuda_stream, ctx=ctx)

        def plain():
            out = []
            for col, s, r in zip(cols, spans, room):
                if col.kind in (1, 4, 8):
                    out.append(torch.cat([col.values[f:f + c] for f, c in ranges]))
                elif col.kind == tabular.OXH_COL_BOOL:   # the bytes that hold the bits
                    out.append(torch.cat([col.values[f >> 3:(f + c + 7) >> 3] for f, c in ranges]))
                elif s is not None:   # one copy of the byte total (the ranges of one frame are contiguous when they cover it)
                    at = 0
                    for lo, hi in s:
                        r[at:at + hi - lo].copy_(col.values[lo:hi])
                        at += hi - lo
                    out.append(r)
            return out

        calls = {"concat": concat, "take": take, "torch": plain}
        for _ in range(2):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(a.reps):   # alternating
            for k, fn in calls.items():
                times[k].append(timed(fn))
        same(times["concat"][-1][2], times["take"][-1][2])
        moved = 0
        for c in times["concat"][-1][2]:
            moved += 2 * sum(t.numel() * t.element_size() for t in (c.values, c.offsets, c.validity) if t is not None)
        m = {k: stats(v) for k, v in times.items()}
        case = {"rows_out": count, "parts": len(ranges), "bytes_read_and_written": moved, **{k: v for k, v in m.items()},
                "gb_per_s": round(moved / (m["concat"]["event_ms_median"] * 1e-3) / 1e9, 1),
                "over_take": round(m["concat"]["event_ms_median"] / m["take"]["event_ms_median"], 3),
                "over_torch": round(m["concat"]["event_ms_median"] / m["torch"]["event_ms_median"], 3)}
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)

    def split(k):
        edges = [n * i // k for i in range(k + 1)]
        return [(lo, hi - lo) for lo, hi in zip(edges[:-1], edges[1:])]

    plans = {"parts1": (frame, split(1)), "parts4": (frame, split(4)), "parts64": (frame, split(64)),
             "head100": (frame, [(0, min(100, n))]), "tail100": (frame, [(n - min(100, n), min(100, n))]),
             "int64": (frame[:1], split(1)), "bool": (frame[2:3], split(1)), "string": (frame[3:4], split(1))}
    for name in a.cases.split(","):
        run_case(name, *plans[name])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
