"""The row filter (oxh_filter_rows_device) at the size of a real table, --rows (10 M) rows of the row-hash probe's
frame (Int64, Float64, Boolean, two strings of 0-48 B) and a column of 100 labels:
  i1 / i50 / i100   one Int64 term `x > v` that selects about 1 %, 50 % and every row;
  label             `label == label-042`, one of 100 labels of 9 bytes;
  chain             `x > v && y < 0.5 || flag == true`, over Int64, Float64 and Boolean;
  mask_only         i50 with idx NULL: no scan, no emit.
Beside every case, in the same run and alternating with it:
  nonzero           `torch.nonzero(x > v)` for the single-term Int64 cases -- what a caller with torch at hand writes;
  bytes             the bytes the call must move -- the columns its terms name, the mask, 4 B per selected row -- at
                    the rate at which this run's `copy_` of a tensor of 8 B per row moves bytes (read + written).
Both ratios go into the JSON; none is fixed in advance. All inputs device-resident, HIP events on the call's
stream around the blocking call (and the host clock), two warm calls, medians of --reps. Every case is checked:
idx is exactly the set bits of the mask, their number is stats.selected, and on a sample of rows the mask's bits
are the restatement's of tests/_filterrows.py over those rows. Which launch takes the time is a matter for
`rocprofv3 --kernel-trace --stats -- python tools/filter_rows_probe.py --reps 3`, in a run of its own.

    python tools/filter_rows_probe.py [--rows 10000000] [--reps 15] [--out profiles/filter_rows/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIGNED, FLOAT = 0, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--cases", default="i1,i50,i100,label,chain,mask_only")
    ap.add_argument("--sample", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_rows", "probe.json"))
    a = ap.parse_args()

    import torch

    import _filterrows
    from oxen_amd import _capi, tabular
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("filter_rows_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    ctx = _capi.Context(0)
    stream = torch.cuda.Stream()
    torch.manual_seed(a.seed)
    n = a.rows
    cases = a.cases.split(",")

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
            sys.exit(f"filter_rows_probe: {what}")

    def strings(m, top):
        lens = torch.randint(0, top + 1, (m,), dtype=torch.int64, device=dev)
        offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        values = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device=dev)
        return Column(tabular.OXH_COL_BYTES32, m, values, offsets.to(torch.int32))

    def host(c):
        np_of = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return Column(c.kind, c.nrows, np_of(c.values), np_of(c.offsets), np_of(c.validity), c.value_bit, c.validity_bit)

    def column_bytes(c):
        return sum(t.numel() * t.element_size() for t in (c.values, c.offsets, c.validity) if t is not None)

    # the frame: the row-hash probe's five columns, and the labels
    x = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev)
    y = torch.randn(n, dtype=torch.float64, device=dev)
    pick = torch.randint(0, 100, (n,), device=dev)
    text = torch.empty((n, 9), dtype=torch.uint8, device=dev)
    text[:, :6] = torch.tensor(list(b"label-"), dtype=torch.uint8, device=dev)
    for k in range(3):
        text[:, 6 + k] = (48 + (pick // 10 ** (2 - k)) % 10).to(torch.uint8)
    frame = [Column(8, n, x), Column(8, n, y),
             Column(tabular.OXH_COL_BOOL, n, torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev)),
             strings(n, 48), strings(n, 48),
             Column(tabular.OXH_COL_BYTES32, n, text.reshape(-1), (torch.arange(n + 1, dtype=torch.int64, device=dev) * 9).to(torch.int32))]
    orders = [SIGNED, FLOAT, SIGNED, SIGNED, SIGNED, SIGNED]
    del text
    torch.cuda.synchronize()

    # the copy rate of this run: a copy of 8 B per row, bytes read + bytes written over its time
    scratch = torch.empty_like(x)
    for _ in range(2):
        timed(lambda: scratch.copy_(x))
    copies = [timed(lambda: scratch.copy_(x)) for _ in range(a.reps)]
    copy_ms = float(np.median([c[0] for c in copies]))
    copy_rate = 2 * 8 * n / (copy_ms * 1e-3)      # bytes per second
    del scratch
    result = {"rows": n, "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "copy": {**stats(copies), "bytes_moved": 16 * n, "gb_per_s": round(copy_rate / 1e9, 1)}, "cases": {}}
    print("copy", json.dumps(result["copy"]), flush=True)

    def verify(name, terms, logical, got):
        """idx is the set bits of the mask, in order; their number is `selected`; a sample of rows agrees with the
        restatement over those rows."""
        mask = got.mask
        if got.idx is not None:
            bits = ((mask[:, None] >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1).reshape(-1)
            need(not bool(bits[n:].any()), f"{name}: mask bits past the rows are set")
            rows = torch.nonzero(bits[:n]).reshape(-1)
            need(rows.numel() == got.stats.selected == got.idx.numel(), f"{name}: {rows.numel()} mask bits, {got.stats}")
            need(bool((rows == got.idx.to(torch.int64)).all()), f"{name}: idx is not the set bits of the mask")
        else:
            need(int(np.unpackbits(mask.cpu().numpy()).sum()) == got.stats.selected, f"{name}: mask bits against {got.stats}")
        sample = torch.unique(torch.randint(0, n, (a.sample,), device=dev))
        taken = tabular.take_device(frame, sample.to(torch.int32), stream=stream.cuda_stream, ctx=ctx)
        cols = [host(c)._replace(validity=None) for c in taken]      # the take writes a bitmap of ones
        want = _filterrows.filter_rows(cols, terms, logical, orders)
        rows = sample.cpu().numpy()
        picked = (mask.cpu().numpy()[rows >> 3] >> (rows & 7).astype(np.uint8)) & 1
        need(np.array_equal(np.nonzero(picked)[0].astype(np.uint32), want.idx), f"{name}: a sample of rows differs from the restatement")

    def run_case(name, terms, logical=(), want_idx=True, beside=None):
        def call():
            return tabular.filter_rows_device(frame, terms, logical, orders, want_mask=True, want_idx=want_idx, stream=stream.cuda_stream, ctx=ctx)

        for _ in range(2):
            call()
            if beside:
                timed(beside)
        mine, other = [], []
        for _ in range(a.reps):   # alternating
            mine.append(timed(call))
            if beside:
                other.append(timed(beside))
        got = mine[-1][2]
        verify(name, terms, list(logical), got)
        named = sorted({t[0] for t in terms})
        must_move = sum(column_bytes(frame[c]) for c in named) + (n + 7) // 8 + (4 * got.stats.selected if want_idx else 0)
        m = stats(mine)
        floor_ms = must_move / copy_rate * 1e3
        case = {**m, "selected": got.stats.selected, "null_rows": got.stats.null_rows, "share_selected": round(got.stats.selected / n, 4),
                "bytes_must_move": must_move, "bytes_at_copy_rate_ms": round(floor_ms, 4),
                "over_bytes_at_copy_rate": round(m["event_ms_median"] / floor_ms, 2),
                "gb_per_s": round(must_move / (m["event_ms_median"] * 1e-3) / 1e9, 1),
                "mrows_per_s": round(n / m["event_ms_median"] / 1e3, 1)}
        if beside:
            o = stats(other)
            need(other[-1][2].numel() == got.stats.selected, f"{name}: torch.nonzero finds {other[-1][2].numel()} rows")
            case["torch_nonzero"] = o
            case["over_torch_nonzero"] = round(m["event_ms_median"] / o["event_ms_median"], 2)
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)

    GT, LT, EQ = _capi.OXH_FILTER_GT, _capi.OXH_FILTER_LT, _capi.OXH_FILTER_EQ
    AND, OR = _capi.OXH_FILTER_AND, _capi.OXH_FILTER_OR
    word = lambda v: v & ((1 << 64) - 1)  # noqa: E731
    span = 1 << 40
    thresholds = {"i1": int(span * 0.98), "i50": 0, "i100": -span - 1}
    for name in ("i1", "i50", "i100"):
        if name in cases:
            v = thresholds[name]
            run_case(name, [(0, GT, word(v))], beside=lambda v=v: torch.nonzero(x > v))
    if "label" in cases:
        run_case("label", [(5, EQ, b"label-042")])
    if "chain" in cases:
        half = struct.unpack("<Q", struct.pack("<d", 0.5))[0]
        run_case("chain", [(0, GT, word(0)), (1, LT, half), (2, EQ, 1)], [AND, OR])
    if "mask_only" in cases:
        run_case("mask_only", [(0, GT, word(0))], want_idx=False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
