"""The grouping of rows (oxh_group_rows_device) at the size of a real table, --rows (10 M) rows of the row-hash
probe's frame (Int64, Float64, Boolean, two strings of 0-48 B):
  a  keyed on all five columns, every row distinct;
  b  the same with 1 % of the rows replaced by copies of other rows;
  d  the same with every row a copy of row 0 (one group: every add of the count on one address);
  c  keyed on one string column of 100 labels, drawn at random: the shape `--unique_count label` exists for.
Beside every case, in the same run and alternating with it, the FLOOR: oxh_row_hashes_device of the same columns
plus one oxh_dedup_index_insert_device of the digests into a fresh index -- entries that exist without this
call, which adds to them the tags of the key image, three passes over the rows and a scan. The floor is timed
with the index made and destroyed inside the window (as the call does with its private one) and outside it.
All inputs device-resident, HIP events on the call's stream around the blocking call (and the host clock), one
warm call, medians of --reps. On a sample of rows the partition the call returns is compared with the
restatement of tests/_grouprows.py over those rows and their groups' first rows, and the case's known totals
are checked. pandas' drop_duplicates / groupby(dropna=False).size() at --cpu-rows is the CPU beside it.
Which launch takes the time is a matter for `rocprofv3 --kernel-trace --stats -- python
tools/group_rows_probe.py --cases c --reps 3 --cpu-rows 0`, in a run of its own.

    python tools/group_rows_probe.py [--rows 10000000] [--reps 5] [--out profiles/group_rows/probe.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIGNED, FLOAT = 0, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cpu-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--cases", default="abdc")
    ap.add_argument("--sample", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_rows", "probe.json"))
    a = ap.parse_args()

    import torch

    import _grouprows
    from oxen_amd import _capi, tabular
    from oxen_amd.dedup import DedupIndex
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("group_rows_probe: no GPU (there is nothing to measure on a CPU)")
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

    def strings(m, top):
        lens = torch.randint(0, top + 1, (m,), dtype=torch.int64, device=dev)
        offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        values = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device=dev)
        return Column(tabular.OXH_COL_BYTES32, m, values, offsets.to(torch.int32))

    def host(c):
        np_of = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return Column(c.kind, c.nrows, np_of(c.values), np_of(c.offsets), np_of(c.validity), c.value_bit, c.validity_bit)

    def sample_check(cols, orders, g, what):
        """The rows of a sample and the first rows of their groups, brought to the host through the take: the
        restatement's partition of those rows is the one `group` says."""
        group = g.group.to(torch.int64)
        if not bool((group <= torch.arange(n, device=dev)).all()) or not bool((group[group] == group).all()):
            sys.exit(f"group_rows_probe: {what}: group is not a row at or before its own that stands for itself")
        if int(g.first_count.to(torch.int64).sum()) != n or g.first_idx.numel() != g.stats.groups:
            sys.exit(f"group_rows_probe: {what}: the groups' sizes do not add up to the rows")
        pick = torch.randint(0, n, (a.sample,), device=dev)
        rows = torch.unique(torch.cat([pick, group[pick]]))
        taken = tabular.take_device(cols, rows.to(torch.int32), stream=stream.cuda_stream, ctx=ctx)
        want = _grouprows.group_rows([host(c) for c in taken], orders)
        got = group[rows].cpu().numpy()
        rows_host = rows.cpu().numpy()
        if not np.array_equal(rows_host[want.group.astype(np.int64)], got):
            sys.exit(f"group_rows_probe: {what}: the partition of a sample differs from the restatement's")
        count = g.count.to(torch.int64)
        if not bool((count[pick] == count[group[pick]]).all()):
            sys.exit(f"group_rows_probe: {what}: a row's count is not its group's")

    result = {"rows": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "cases": {}}

    def run_case(name, cols, orders, expect):
        def call():
            return tabular.group_rows_device(cols, orders, stream=stream.cuda_stream, ctx=ctx)

        def floor(own_index):
            def fn():
                index = own_index or DedupIndex(ctx, capacity=n)
                h = tabular.row_hashes_device(cols, stream=stream.cuda_stream, ctx=ctx)
                index.insert_device(h, stream=stream.cuda_stream)
                if not own_index:
                    index.close()
            return fn

        call()
        floor(None)()
        mine, with_index, bare = [], [], []
        for _ in range(a.reps):   # alternating
            mine.append(timed(call))
            with_index.append(timed(floor(None)))
            index = DedupIndex(ctx, capacity=n)
            bare.append(timed(floor(index)))
            index.close()
        g = mine[-1][2]
        expect(g)
        sample_check(cols, orders, g, name)
        m, f, b = stats(mine), stats(with_index), stats(bare)
        case = {**m, "groups": g.stats.groups, "duplicated": g.stats.duplicated, "largest": g.stats.largest, "long_rows": g.stats.long_rows,
                "floor_hashes_plus_insert": f, "floor_index_made_outside": b,
                "over_floor": round(m["event_ms_median"] / f["event_ms_median"], 2),
                "over_floor_index_made_outside": round(m["event_ms_median"] / b["event_ms_median"], 2),
                "mrows_per_s": round(n / m["event_ms_median"] / 1e3, 1)}
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)

    def need(cond, what):
        if not cond:
            sys.exit(f"group_rows_probe: {what}")

    orders5 = [SIGNED, FLOAT, SIGNED, SIGNED, SIGNED]
    if any(c in a.cases for c in "abd"):
        base = [Column(8, n, torch.randperm(n, device=dev).to(torch.int64) * 7919 - (n * 7919) // 2),     # unique: every row distinct
                Column(8, n, torch.randn(n, dtype=torch.float64, device=dev)),
                Column(tabular.OXH_COL_BOOL, n, torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev)),
                strings(n, 48), strings(n, 48)]
        torch.cuda.synchronize()
        if "a" in a.cases:
            run_case("a_all_distinct", base, orders5, lambda g: need(g.stats[:3] == (n, 0, 1), f"a: {g.stats}"))
        if "b" in a.cases:
            idx = torch.arange(n, dtype=torch.int64, device=dev)
            dup = torch.rand(n, device=dev) < 0.01
            idx[dup] = torch.randint(0, n, (int(dup.sum()),), device=dev)
            cols = tabular.take_device(base, idx.to(torch.int32), stream=stream.cuda_stream, ctx=ctx)
            cols = [c._replace(validity=None) for c in cols]     # the take writes a bitmap of ones
            expected_groups = int(torch.unique(idx).numel())
            run_case("b_one_percent_duplicated", cols, orders5,
                     lambda g: need(g.stats.groups == expected_groups and g.stats.duplicated > 0, f"b: {g.stats} for {expected_groups} source rows"))
            del cols, idx, dup
        if "d" in a.cases:
            cols = tabular.take_device(base, torch.zeros(n, dtype=torch.int32, device=dev), stream=stream.cuda_stream, ctx=ctx)
            cols = [c._replace(validity=None) for c in cols]
            run_case("d_all_equal", cols, orders5, lambda g: need(g.stats[:3] == (1, n, n), f"d: {g.stats}"))
            del cols
        del base
        torch.cuda.empty_cache()

    if "c" in a.cases:
        labels = 100
        pick = torch.randint(0, labels, (n,), device=dev)
        values = torch.empty((n, 9), dtype=torch.uint8, device=dev)
        values[:, :6] = torch.tensor(list(b"label-"), dtype=torch.uint8, device=dev)
        for k in range(3):
            values[:, 6 + k] = (48 + (pick // 10 ** (2 - k)) % 10).to(torch.uint8)
        col = Column(tabular.OXH_COL_BYTES32, n, values.reshape(-1), (torch.arange(n + 1, dtype=torch.int64, device=dev) * 9).to(torch.int32))
        torch.cuda.synchronize()
        sizes = torch.bincount(pick, minlength=labels)

        def expect(g):
            need(g.stats.groups == labels and g.stats.duplicated == n, f"c: {g.stats}")
            first = g.first_idx.to(torch.int64)
            need(bool((g.first_count.to(torch.int64) == sizes[pick[first]]).all()), "c: first_count is not the labels' sizes")

        run_case("c_one_string_column_100_labels", [col], [SIGNED], expect)
        del pick, values, col
        torch.cuda.empty_cache()

    if a.cpu_rows:
        try:
            import pandas as pd
        except ImportError:
            pd = None
        if pd is not None:
            rng = np.random.default_rng(a.seed)
            m = a.cpu_rows

            def words():
                lens = rng.integers(0, 49, size=m)
                at = np.cumsum(lens) - lens
                text = rng.integers(97, 123, size=int(lens.sum()), dtype=np.uint8).tobytes().decode()
                return [text[o:o + l] for o, l in zip(at.tolist(), lens.tolist())]

            df = pd.DataFrame({"i": rng.permutation(m).astype(np.int64), "f": rng.standard_normal(m), "b": rng.random(m) < 0.5,
                               "s": words(), "t": words()})
            lab = pd.DataFrame({"label": ["label-%03d" % k for k in rng.integers(0, 100, size=m)]})
            t0 = time.perf_counter()
            df.drop_duplicates()
            t1 = time.perf_counter()
            lab.groupby("label", dropna=False, sort=False).size()
            t2 = time.perf_counter()
            result["cpu"] = {"rows": m, "pandas": pd.__version__, "drop_duplicates_all_distinct_5_columns_ms": round((t1 - t0) * 1e3, 1),
                             "groupby_size_100_labels_ms": round((t2 - t1) * 1e3, 1)}
            print("cpu", json.dumps(result["cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
