"""The take of the joined rows' columns (oxh_take_columns_device) at the size of a real table: the keyed-diff
probe's case -- --rows (10 M) rows per side, unique keys, 1 % removed, 1 % modified, 1 % added, the right side
in the left's order ("kept") and shuffled -- and, through the pairs that diff emits, the row-hash probe's frame
on each side: Int64, Float64, Boolean and two strings of mean 24 B. The pairs are taken twice: the emitted ones
("changed", about 3 % of the rows: what `oxen diff` shows) and all joined rows ("all", the diff with
OXH_KEYED_DIFF_KEEP_UNCHANGED: the gather at full size). Also one 1 M-row column of 2 KiB strings, permuted.

Recorded per case, all inputs device-resident, HIP events on the call's stream around the blocking call (and
the host clock), one warm call, medians of --reps, the forms alternating:
  take           the second call (capacity known), every column of the plan;
  sizes          the sizes-only call;
  fixed          the second call over the fixed-width columns alone, and beside it
  index_select   torch.index_select on the same device tensors with the same indices (absent ones clamped to
                 row 0, outside the clock): the device yardstick for the gather itself;
  pyarrow        take + coalesce of the same columns on the host at --cpu-rows, the CPU beside it;
  bytes          sources read plus outputs written by the take (from the shapes), over the event time,
                 against the 8.0 TB/s HBM peak.
--sweep: the short / long threshold T and the piece size P over a small grid (oxh_set_kernel_variant, a
test-only hook) on the "all" pairs and on the 2 KiB column; the grid and the times go into the JSON.
--e2e: `diff_dfs_contents` on host frames of --cpu-rows rows against row hashes + keyed diff + pyarrow take.

    python tools/take_probe.py [--rows 10000000] [--reps 5] [--sweep] [--e2e] [--out profiles/take/probe.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
THRESHOLDS = [0, 32, 64, 128, 256, 512, 1024, 4096]      # kTakeThresholds, take_columns.hip
PIECES = [256, 512, 1024, 2048, 4096, 8192, 16384, 65536]  # kTakePieces
VARIANT = 9100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--long-rows", type=int, default=1_000_000)
    ap.add_argument("--cpu-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "take", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("take_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    ctx = _capi.Context(0)
    L = _capi.lib()
    stream = torch.cuda.Stream()
    torch.manual_seed(a.seed)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record(stream)
        fn()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3

    def stats(xs):
        ev = [x[0] for x in xs]
        return {"event_ms_median": round(float(np.median(ev)), 3), "event_ms_min": round(min(ev), 3), "event_ms_max": round(max(ev), 3),
                "call_ms_median": round(float(np.median([x[1] for x in xs])), 3)}

    def digests(n):
        return torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), dtype=torch.int64, device=dev)

    def string_column(n, mean, kind=32):
        lens = torch.randint(0, 2 * mean + 1, (n,), dtype=torch.int64, device=dev)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        total = int(offsets[-1])
        values = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
        return Column(kind, n, values, offsets.to(torch.int32) if kind == 32 else offsets)

    def frame(n):
        """Int64 (with nulls), Float64, Boolean, two strings of mean 24 B (the second with nulls)."""
        bitmap = lambda: torch.randint(1, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev)  # noqa: E731
        s2 = string_column(n, 24)
        return [Column(8, n, torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev), None, bitmap()),
                Column(8, n, torch.randn(n, dtype=torch.float64, device=dev)),
                Column(16, n, torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev)),
                string_column(n, 24), s2._replace(validity=bitmap())]

    def tables(n, shuffled):
        lk, lt = digests(n), digests(n)
        gone = torch.rand(n, device=dev) < 0.01
        rk, rt = lk[~gone].clone(), lt[~gone].clone()
        changed = torch.rand(rk.shape[0], device=dev) < 0.01
        rt[changed] = digests(int(changed.sum()))
        extra = n // 100
        rk, rt = torch.cat([rk, digests(extra)]), torch.cat([rt, digests(extra)])
        if shuffled:
            order = torch.randperm(rk.shape[0], device=dev)
            rk, rt = rk[order].contiguous(), rt[order].contiguous()
        return lk, lt, rk, rt

    class Take:
        """One take over device columns, as the raw ABI takes it; the outputs are made once, outside the clock."""

        def __init__(self, cols, idx0, idx1, plan):
            self.keep = (cols, idx0, idx1)
            torch.cuda.synchronize()   # the inputs were made on torch's stream
            self.n = int((idx0 if idx0 is not None else idx1).numel())
            ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
            rows, words, self.plan, self.kinds = tabular._take_tables(cols, plan)
            self.head = (ctx.handle, len(cols), *tabular._tables(cols, ptr), rows, self.n, ptr(idx0), ptr(idx1), len(self.plan), words)
            self.value_bytes = (ctypes.c_uint64 * len(self.plan))()
            self.written = ctypes.c_uint32(0)
            self.sizes()
            self.need = list(self.value_bytes)
            self.outs = [[torch.empty(size, dtype=torch.uint8, device=dev) for size in sizes]
                         for sizes in tabular._take_sizes(self.kinds, self.n, self.value_bytes)]
            self.capacity = (ctypes.c_uint64 * len(self.plan))(*self.need)
            self.arrays = [tabular._pointers([ptr(o[k]) for o in self.outs]) for k in range(3)]
            # what the take reads and writes, from the shapes: both index arrays; per column the output buffers, and
            # as many source bytes as it writes values (plus a source offset pair per row of a byte column)
            self.bytes = 8 * self.n
            for kind, sizes in zip(self.kinds, tabular._take_sizes(self.kinds, self.n, self.value_bytes)):
                self.bytes += 2 * sizes[0] + sizes[1] + sizes[2] + (sizes[1] if kind in (32, 64) else 0)
            torch.cuda.synchronize()

        def sizes(self):
            _capi.check(L.oxh_take_columns_device(*self.head, None, None, None, None, self.value_bytes, ctypes.byref(self.written),
                                                  stream.cuda_stream), "oxh_take_columns_device")

        def __call__(self):
            _capi.check(L.oxh_take_columns_device(*self.head, self.capacity, *self.arrays, self.value_bytes,
                                                  ctypes.byref(self.written), stream.cuda_stream), "oxh_take_columns_device")
            if not self.written.value:
                sys.exit("take_probe: the second call did not write")

    def rate(nbytes, s):
        return {"bytes": int(nbytes), "GB_per_s": round(nbytes / (s["event_ms_median"] * 1e-3) / 1e9, 1),
                "share_of_hbm_peak": round(nbytes / (s["event_ms_median"] * 1e-3) / HBM_PEAK, 3)}

    def sweep(take, thresholds, pieces):
        grid = []
        for p in pieces:
            for t in thresholds:
                L.oxh_set_kernel_variant(VARIANT + 8 * PIECES.index(p) + THRESHOLDS.index(t))
                take()
                xs = [timed(take) for _ in range(a.reps)]
                grid.append({"T": t, "P": p, **stats(xs)})
        L.oxh_set_kernel_variant(0)
        return grid

    result = {"rows_each": a.rows, "reps": a.reps, "device": torch.cuda.get_device_name(0), "hbm_peak_B_per_s": HBM_PEAK, "orders": {}}
    for order in ("kept", "shuffled"):
        lk, lt, rk, rt = tables(a.rows, order == "shuffled")
        nl, nr = lk.shape[0], rk.shape[0]
        left, right = frame(nl), frame(nr)
        cols = left + right
        k = len(left)
        plan = [(k + 0, 1, 0, 0), (1, 0, None, 0), (k + 1, 1, None, 0), (2, 0, None, 0), (k + 2, 1, None, 0),
                (3, 0, None, 0), (k + 3, 1, None, 0), (4, 0, None, 0), (k + 4, 1, None, 0)]
        fixed_plan = [(0, 0, None, 0), (k + 0, 1, None, 0), (1, 0, None, 0), (k + 1, 1, None, 0)]
        torch.cuda.synchronize()
        row = {"nleft": nl, "nright": nr}
        for which, keep in (("changed", False), ("all", True)):
            d = tabular.keyed_diff_digests_device(lk, rk, lt, rt, keep_unchanged=keep, stream=stream.cuda_stream, ctx=ctx)
            i0, i1 = d.left_rows.contiguous(), d.right_rows.contiguous()
            whole, fixed = Take(cols, i0, i1, plan), Take(cols, i0, i1, fixed_plan)
            # the yardstick: the same four gathers by torch, absent rows clamped to row 0
            c0, c1 = i0.clamp(min=0).to(torch.int64), i1.clamp(min=0).to(torch.int64)
            srcs = [(left[0].values, c0), (right[0].values, c1), (left[1].values, c0), (right[1].values, c1)]
            dsts = [torch.empty(whole.n, dtype=s.dtype, device=dev) for s, _ in srcs]
            torch.cuda.synchronize()

            def index_select():
                with torch.cuda.stream(stream):
                    for (s, i), o in zip(srcs, dsts):
                        torch.index_select(s, 0, i, out=o)

            # the int32 indices as they are (torch converts nothing): index_select takes int32 too
            s32 = [(s, i.to(torch.int32)) for s, i in srcs]

            def index_select32():
                with torch.cuda.stream(stream):
                    for (s, i), o in zip(s32, dsts):
                        torch.index_select(s, 0, i, out=o)

            whole(), fixed(), index_select(), index_select32()   # warm
            # the fixed-width take gives what torch gives wherever the row is present
            # (the Float64 column, which has no nulls of its own)
            got = fixed.outs[2][0].view(torch.int64)
            present = i0 >= 0
            if not torch.equal(got[present], dsts[2].view(torch.int64)[present]):
                sys.exit("take_probe: the take and index_select differ")
            t_take, t_sizes, t_fixed, t_sel, t_sel32 = [], [], [], [], []
            for _ in range(a.reps):   # alternating
                t_take.append(timed(whole))
                t_sizes.append(timed(whole.sizes))
                t_fixed.append(timed(fixed))
                t_sel.append(timed(index_select))
                t_sel32.append(timed(index_select32))
            case = {"pairs": whole.n, "take": {**stats(t_take), **rate(whole.bytes, stats(t_take))}, "sizes_only": stats(t_sizes),
                    "fixed": {**stats(t_fixed), **rate(fixed.bytes, stats(t_fixed))}, "index_select_int64_idx": stats(t_sel),
                    "index_select_int32_idx": stats(t_sel32), "value_bytes": whole.need}
            case["fixed_over_index_select"] = round(case["fixed"]["event_ms_median"] /
                                                    min(case["index_select_int64_idx"]["event_ms_median"],
                                                        case["index_select_int32_idx"]["event_ms_median"]), 2)
            if a.sweep and which == "all" and order == "shuffled":
                case["sweep"] = sweep(whole, [32, 64, 128, 256, 4096], [4096])
            row[which] = case
            print(order, which, json.dumps(case), flush=True)
            del whole, fixed, dsts, srcs, s32, c0, c1, i0, i1, d
        result["orders"][order] = row
        del lk, lt, rk, rt, left, right, cols
        torch.cuda.empty_cache()

    # one column of 2 KiB strings, permuted
    n = a.long_rows
    col = string_column(n, 2048, kind=64)
    perm = torch.randperm(n, device=dev).to(torch.int32)
    long_take = Take([col], perm, None, None)
    long_take()
    xs = []
    for _ in range(a.reps):
        xs.append(timed(long_take))
    result["long_strings"] = {"rows": n, "mean_bytes": 2048, "take": {**stats(xs), **rate(long_take.bytes, stats(xs))},
                              "value_bytes": long_take.need}
    if a.sweep:
        result["long_strings"]["sweep"] = sweep(long_take, [256, 1024, 4096], [512, 1024, 2048, 4096, 16384, 65536])
    print("long", json.dumps(result["long_strings"]), flush=True)
    del long_take, col, perm
    torch.cuda.empty_cache()

    if a.cpu_rows:
        result["cpu"] = cpu_leg(a, ctx, a.e2e)
        print("cpu", json.dumps(result["cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


def cpu_leg(a, ctx, e2e):
    """pyarrow take + coalesce of the same kind of frame on the host at --cpu-rows; with --e2e the whole
    `diff_dfs_contents` against row hashes + keyed diff + that pyarrow take."""
    import pyarrow as pa
    import pyarrow.compute as pc

    from oxen_amd import tabular

    n = a.cpu_rows
    rng = np.random.default_rng(a.seed)

    def table(ids, seed):
        r = np.random.default_rng(seed)
        m = len(ids)
        words = pa.array(["%024x" % v for v in r.integers(0, 1 << 62, size=m).tolist()])
        return pa.table({"id": pa.array(ids), "x": pa.array(r.standard_normal(m)), "flag": pa.array(r.random(m) < 0.5),
                         "s1": words, "s2": words.take(pa.array(r.permutation(m)))})

    ids = rng.permutation(2 * n)[:n].astype(np.int64)
    keep = rng.permutation(n)[: n - n // 100]
    left = table(ids, 1)
    right_ids = np.concatenate([ids[keep], 4 * n + np.arange(n // 100)])
    right = table(right_ids, 1)   # the same generator: rows with equal position differ, so most pairs are modified
    fl, fr = tabular.columns_from_arrow(left), tabular.columns_from_arrow(right)
    t0 = time.perf_counter()
    d, contents = tabular.diff_dfs_contents(fl, fr, keys=["id"], targets=["x", "s1"], ctx=ctx)
    t_ours = time.perf_counter() - t0
    t0 = time.perf_counter()
    d2 = tabular.diff_dfs(fl, fr, keys=["id"], targets=["x", "s1"], ctx=ctx)
    t_diff = time.perf_counter() - t0
    as_index = lambda i: pa.array(np.where(i < 0, 0, i).astype(np.uint32), mask=i < 0)  # noqa: E731
    t0 = time.perf_counter()
    li, ri = as_index(d2.left_rows), as_index(d2.right_rows)
    out = {"id": pc.coalesce(right.column("id").take(ri), left.column("id").take(li))}
    for name in ("x", "s1"):
        out[name + ".left"], out[name + ".right"] = left.column(name).take(li), right.column(name).take(ri)
    t_arrow = time.perf_counter() - t0
    t0 = time.perf_counter()
    tabular.take(list(fl.values()) + list(fr.values()), d2.left_rows, d2.right_rows,
                 [(5, 1, 0, 0), (1, 0, None, 0), (6, 1, None, 0), (3, 0, None, 0), (8, 1, None, 0)], ctx=ctx)
    t_take_host = time.perf_counter() - t0
    schema = pa.schema([("id", pa.int64()), ("x.left", pa.float64()), ("x.right", pa.float64()), ("s1.left", pa.string()), ("s1.right", pa.string())])
    ours = tabular.columns_to_arrow(contents, schema)
    for name in schema.names:
        theirs = out[name].combine_chunks() if isinstance(out[name], pa.ChunkedArray) else out[name]
        if not ours.column(name).combine_chunks().equals(theirs):
            sys.exit(f"take_probe: column {name} differs from pyarrow's")
    leg = {"rows_each": n, "pairs": int(len(d2.left_rows)), "pyarrow": pa.__version__, "pyarrow_take_coalesce_s": round(t_arrow, 4),
           "take_host_form_s": round(t_take_host, 4)}
    if e2e:
        leg.update({"diff_dfs_contents_s": round(t_ours, 4), "diff_dfs_s": round(t_diff, 4),
                    "diff_dfs_plus_pyarrow_take_s": round(t_diff + t_arrow, 4)})
    return leg


if __name__ == "__main__":
    main()
