"""The stable row sort (oxh_sort_rows_device) at the size of a real table, --rows (10 M) rows:
  a  one shuffled unique int64 key, beside torch.sort(stable=True) of the same tensor (the device yardstick: a
     single-launch-per-pass onesweep with look-back, which this design gives up on purpose);
  b  the same keys already in order;
  c  the keyed-diff probe's joined rows (unique keys, 1 % removed, 1 % modified, 1 % added, the right side
     shuffled, all joined rows kept) sorted on their int64 key, end to end through the device steps of
     `diff_contents(sort=True)`: the take of the coalesced key, the sort, the take of the pairs and the status;
  d  unique string keys of mean 24 B behind a 13-byte common prefix;
  e  a key of 16 distinct values followed by an int64 key.
All inputs device-resident, HIP events on the call's stream around the blocking call (and the host clock), one
warm call, medians of --reps, the forms alternating, every permutation checked on a sample (the keys at
consecutive places do not decrease; stable where they are equal). numpy's lexsort / argsort(kind="stable") at
--cpu-rows is the CPU beside it. Which launch takes the time is a matter for `rocprofv3 --kernel-trace --stats --
python tools/sort_rows_probe.py --cases a --reps 3 --cpu-rows 0`, in a run of its own
(profiles/sort_rows/probe_kernel_stats.csv keeps its kernel rows, names shortened).

    python tools/sort_rows_probe.py [--rows 10000000] [--reps 5] [--out profiles/sort_rows/probe.json]
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
SIGNED = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cpu-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_rows", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("sort_rows_probe: no GPU (there is nothing to measure on a CPU)")
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
        out = fn()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3, out

    def stats(xs):
        ev = [x[0] for x in xs]
        return {"event_ms_median": round(float(np.median(ev)), 3), "event_ms_min": round(min(ev), 3), "event_ms_max": round(max(ev), 3),
                "call_ms_median": round(float(np.median([x[1] for x in xs])), 3)}

    def sort(cols, orders):
        return tabular.sort_indices_device(cols, orders, stream=stream.cuda_stream, ctx=ctx)

    def sample_check(perm, keys, what):
        """keys: int64 device tensors, most significant first. On a sample of adjacent places: the keys do not
        decrease, and where they are all equal the rows ascend (stable)."""
        p = perm.to(torch.int64)
        at = torch.randint(0, p.numel() - 1, (min(200_000, p.numel() - 1),), device=dev)
        x, y = p[at], p[at + 1]
        less = torch.zeros_like(at, dtype=torch.bool)
        equal = torch.ones_like(at, dtype=torch.bool)
        for k in keys:
            less |= equal & (k[x] < k[y])
            equal &= k[x] == k[y]
        if not bool((less | (equal & (x < y))).all()):
            sys.exit(f"sort_rows_probe: {what}: the permutation is not the stable sort on a sample")
        if not bool((torch.bincount(p, minlength=p.numel()) == 1).all()):
            sys.exit(f"sort_rows_probe: {what}: not a permutation of the rows")

    def measure(fn, other=None):
        fn()
        if other:
            other()
        mine, theirs = [], []
        for _ in range(a.reps):   # alternating
            mine.append(timed(fn))
            if other:
                theirs.append(timed(other))
        return mine, theirs

    result = {"rows": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "cases": {}}

    def record(name, xs, st, extra=None):
        case = {**stats(xs), "rounds": st.rounds, "passes": st.passes, "tied": st.tied, **(extra or {})}
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)

    if "a" in a.cases or "b" in a.cases:
        keys = torch.randperm(n, device=dev).to(torch.int64) * 7919 - (n * 7919) // 2    # unique, both signs
        col = Column(8, n, keys)
        torch.cuda.synchronize()

        def torch_sort():
            with torch.cuda.stream(stream):
                return torch.sort(keys, stable=True)

        if "a" in a.cases:
            mine, theirs = measure(lambda: sort([col], [SIGNED]), torch_sort)
            perm, st = mine[-1][2]
            sample_check(perm, [keys], "a")
            if not torch.equal(perm.to(torch.int64), theirs[-1][2][1]):
                sys.exit("sort_rows_probe: a: differs from torch.sort(stable=True)")
            t = stats(theirs)
            ratio = stats(mine)["event_ms_median"] / t["event_ms_median"]
            record("a_shuffled_unique_int64", mine, st, {"torch_sort_stable": t, "over_torch_sort": round(ratio, 2),
                                                         "spread_ms": round(stats(mine)["event_ms_max"] - stats(mine)["event_ms_min"], 3),
                                                         "torch_spread_ms": round(t["event_ms_max"] - t["event_ms_min"], 3)})
        if "b" in a.cases:
            ordered = Column(8, n, torch.sort(keys).values.contiguous())
            torch.cuda.synchronize()
            mine, _ = measure(lambda: sort([ordered], [SIGNED]))
            perm, st = mine[-1][2]
            if not torch.equal(perm, torch.arange(n, dtype=torch.int32, device=dev)):
                sys.exit("sort_rows_probe: b: sorted keys must give the identity")
            record("b_ordered_int64", mine, st)
        del keys, col
        torch.cuda.empty_cache()

    if "c" in a.cases:
        def digests(m):
            return torch.randint(-(1 << 63), (1 << 63) - 1, (m, 2), dtype=torch.int64, device=dev)

        lk, lt = digests(n), digests(n)
        gone = torch.rand(n, device=dev) < 0.01
        rk, rt = lk[~gone].clone(), lt[~gone].clone()
        changed = torch.rand(rk.shape[0], device=dev) < 0.01
        rt[changed] = digests(int(changed.sum()))
        extra = n // 100
        rk, rt = torch.cat([rk, digests(extra)]), torch.cat([rt, digests(extra)])
        order = torch.randperm(rk.shape[0], device=dev)
        rk, rt = rk[order].contiguous(), rt[order].contiguous()
        # the key column of each frame: the low word of its key digest (unique with these rows)
        left = {"id": Column(8, n, lk[:, 0].contiguous())}
        right = {"id": Column(8, rk.shape[0], rk[:, 0].contiguous())}
        torch.cuda.synchronize()
        d = tabular.keyed_diff_digests_device(lk, rk, lt, rt, keep_unchanged=True, stream=stream.cuda_stream, ctx=ctx)
        d = d._replace(left_rows=d.left_rows.contiguous(), right_rows=d.right_rows.contiguous(), status=d.status.contiguous())
        steps = lambda: tabular.sort_diff_rows_device(left, right, d, ["id"], [SIGNED], stream=stream.cuda_stream, ctx=ctx)  # noqa: E731
        mine, _ = measure(steps)
        got = mine[-1][2]
        l, r = got.left_rows.to(torch.int64), got.right_rows.to(torch.int64)
        key = torch.where(r >= 0, right["id"].values[r.clamp(min=0)], left["id"].values[l.clamp(min=0)])
        if not bool((key[1:] >= key[:-1]).all()):
            sys.exit("sort_rows_probe: c: the joined rows are not in key order")
        case = {**stats(mine), "pairs": int(l.numel())}
        result["cases"]["c_joined_rows_end_to_end"] = case
        print("c", json.dumps(case), flush=True)
        del lk, lt, rk, rt, d, got, l, r, key, left, right
        torch.cuda.empty_cache()

    if "d" in a.cases:
        # unique strings: a 13-byte common prefix, then the row's number in 11 digits (a shuffled order), then
        # padding of 0-24 bytes: mean 36 B in all, 24 B behind the prefix
        ids = torch.randperm(n, device=dev)
        pad = torch.randint(0, 25, (n,), device=dev)
        lens = 13 + 11 + pad
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        values = torch.full((int(offsets[-1]),), 120, dtype=torch.uint8, device=dev)
        prefix = torch.tensor(list(b"common/prefix"), dtype=torch.uint8, device=dev)
        for k in range(13):
            values[offsets[:-1] + k] = prefix[k]
        rest = ids.clone()
        for k in range(10, -1, -1):
            values[offsets[:-1] + 13 + k] = (48 + rest % 10).to(torch.uint8)
            rest //= 10
        col = Column(64, n, values, offsets)
        torch.cuda.synchronize()
        mine, _ = measure(lambda: sort([col], [SIGNED]))
        perm, st = mine[-1][2]
        sample_check(perm, [ids.to(torch.int64)], "d")       # the digits order the cells as the numbers do
        record("d_unique_strings_common_prefix", mine, st, {"mean_bytes": round(float(lens.float().mean()), 1), "prefix_bytes": 13})
        del ids, pad, lens, offsets, values, col, rest
        torch.cuda.empty_cache()

    if "e" in a.cases:
        few = torch.randint(0, 16, (n,), dtype=torch.int32, device=dev)
        wide = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
        cols = [Column(4, n, few), Column(8, n, wide)]
        torch.cuda.synchronize()
        mine, _ = measure(lambda: sort(cols, [SIGNED, SIGNED]))
        perm, st = mine[-1][2]
        sample_check(perm, [few.to(torch.int64), wide], "e")
        record("e_16_values_then_int64", mine, st)
        del few, wide, cols
        torch.cuda.empty_cache()

    if a.cpu_rows:
        rng = np.random.default_rng(a.seed)
        m = a.cpu_rows
        k = rng.permutation(m).astype(np.int64)
        few, wide = rng.integers(0, 16, size=m).astype(np.int32), rng.integers(-2**62, 2**62, size=m).astype(np.int64)
        t0 = time.perf_counter()
        np.argsort(k, kind="stable")
        t1 = time.perf_counter()
        np.lexsort((wide, few))
        t2 = time.perf_counter()
        result["cpu"] = {"rows": m, "numpy": np.__version__, "argsort_stable_int64_ms": round((t1 - t0) * 1e3, 1),
                         "lexsort_16_values_then_int64_ms": round((t2 - t1) * 1e3, 1)}
        print("cpu", json.dumps(result["cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
