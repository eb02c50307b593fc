"""The keyed tabular diff of two device-resident sets of digest tables (oxh_keyed_diff_device) at the size of
a real table: --rows (10 M) rows per side, unique keys, 1 % of the left rows removed, 1 % of the rest with
changed targets, 1 % added. Recorded, for the right side in the left's order ("kept": the removed rows
dropped, the added ones appended) and in a random order ("shuffled"):

  (a) keyed     oxh_keyed_diff_device as shipped, room for nleft + nright pairs: two index inserts, count,
                plan, bucket, classify, the scan's three launches, fill;
  (b) row_diff  oxh_row_diff_device on the same two key tables, which does a subset of that work (the
                inserts, one mark, one flag pass);
  (c) cpu       the same join restated on the CPU at --cpu-rows (1 M) rows per side: pandas' outer merge on the
                key digests' hex strings and the status rule in numpy (the dict restatement of
                tests/_keyeddiff.py where pandas is not importable); its counts must equal the device's.

(a) and (b) alternate in one process; one warm call each first; medians of --reps. Times are HIP events on
the call's stream around the blocking call, and the host clock around it (the call allocates, and reads its
control words back, so the host clock is the larger). The output arrays are made once, outside the clock.
Which launch takes the time is a matter for `rocprofv3 --kernel-trace --stats -- python tools/keyed_diff_probe.py
--reps 2 --cpu-rows 0 --out /dev/null`.

    python tools/keyed_diff_probe.py [--rows 10000000] [--reps 5] [--out profiles/keyed_diff/probe.json]
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
    ap.add_argument("--cpu-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyed_diff", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi

    if not torch.cuda.is_available():
        sys.exit("keyed_diff_probe: no GPU (there is nothing to measure on a CPU)")
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
        out = fn()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3, out

    def med(xs, k):
        return round(float(np.median([x[k] for x in xs])), 3)

    def digests(n):
        return torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), dtype=torch.int64, device=dev)

    def tables(n, shuffled):
        """(left keys, left targets, right keys, right targets, (added, removed, modified))"""
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
        return lk, lt, rk, rt, (extra, int(gone.sum()), int(changed.sum()))

    result = {"rows_each": a.rows, "reps": a.reps, "device": torch.cuda.get_device_name(0), "orders": {}}
    for order in ("kept", "shuffled"):
        lk, lt, rk, rt, (added, removed, modified) = tables(a.rows, order == "shuffled")
        nl, nr = lk.shape[0], rk.shape[0]
        left = torch.empty(nl + nr, dtype=torch.int32, device=dev)
        right = torch.empty(nl + nr, dtype=torch.int32, device=dev)
        status = torch.empty(nl + nr, dtype=torch.uint8, device=dev)
        flags_removed = torch.empty(nl, dtype=torch.uint8, device=dev)
        flags_added = torch.empty(nr, dtype=torch.uint8, device=dev)
        bits = np.zeros(2, dtype=np.uint64)
        counts8, counts2 = np.zeros(8, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        torch.cuda.synchronize()

        def keyed():
            _capi.check(L.oxh_keyed_diff_device(ctx.handle, lk.data_ptr(), nl, rk.data_ptr(), nr, lt.data_ptr(), rt.data_ptr(), None,
                                                None, bits.ctypes.data_as(_capi._u64p), 0, nl + nr, left.data_ptr(),
                                                right.data_ptr(), status.data_ptr(), counts8.ctypes.data_as(_capi._u64p),
                                                stream.cuda_stream), "oxh_keyed_diff_device")

        def row_diff():
            _capi.check(L.oxh_row_diff_device(ctx.handle, lk.data_ptr(), nl, rk.data_ptr(), nr, flags_removed.data_ptr(),
                                              flags_added.data_ptr(), counts2.ctypes.data_as(_capi._u64p), stream.cuda_stream),
                        "oxh_row_diff_device")

        keyed()     # warm: code objects
        row_diff()
        want = [added + removed + modified, added, removed, modified, nl - removed - modified, 0, 0, added + removed + modified]
        if counts8.tolist() != want or counts2.tolist() != [removed, added]:
            sys.exit(f"keyed_diff_probe: {order}: counts {counts8.tolist()} / {counts2.tolist()}, expected {want}")
        kd, rd = [], []
        for _ in range(a.reps):  # alternating
            kd.append(timed(keyed))
            rd.append(timed(row_diff))
        row = {"nleft": nl, "nright": nr, "added": added, "removed": removed, "modified": modified,
               "keyed_event_ms_median": med(kd, 0), "keyed_event_ms_min": round(min(x[0] for x in kd), 3),
               "keyed_call_ms_median": med(kd, 1),
               "row_diff_event_ms_median": med(rd, 0), "row_diff_event_ms_min": round(min(x[0] for x in rd), 3),
               "row_diff_call_ms_median": med(rd, 1),
               "keyed_over_row_diff": round(med(kd, 0) / med(rd, 0), 2),
               "keyed_rows_per_s": round((nl + nr) / (med(kd, 1) * 1e-3))}
        result["orders"][order] = row
        print(order, json.dumps(row), flush=True)
        del lk, lt, rk, rt, left, right, status
    if a.cpu_rows:
        result["cpu"] = cpu_leg(*tables(a.cpu_rows, True)[:4], ctx)
        print("cpu", json.dumps(result["cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


def cpu_leg(lk, lt, rk, rt, ctx):
    """The same kind of tables (shuffled) joined on the CPU; the counts are checked against the library's."""
    from oxen_amd import tabular

    host = [t.cpu().numpy().view(np.uint64) for t in (lk, lt, rk, rt)]
    n = host[0].shape[0]
    d = tabular.keyed_diff_digests(host[0], host[2], host[1], host[3], ctx=ctx)
    hexes = [["%x" % ((hi << 64) | lo) for lo, hi in t.tolist()] for t in (host[0], host[2])]
    try:
        import pandas as pd
    except ImportError:
        pd = None
    t0 = time.perf_counter()
    if pd is not None:
        a = pd.DataFrame({"k": hexes[0], "l": np.arange(n)})
        b = pd.DataFrame({"k": hexes[1], "r": np.arange(len(hexes[1]))})
        m = pd.merge(a, b, on="k", how="outer")
        t1 = time.perf_counter()
        l, r = m["l"].to_numpy(), m["r"].to_numpy()
        both = ~np.isnan(l) & ~np.isnan(r)
        li, ri = l[both].astype(np.int64), r[both].astype(np.int64)
        differ = (host[1][li] != host[3][ri]).any(axis=1)
        got = (int(np.isnan(l).sum()), int(np.isnan(r).sum()), int(differ.sum()), int((~differ).sum()))
        how = "pandas %s outer merge on hex strings" % pd.__version__
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _keyeddiff

        rows = lambda t: [tuple(x) for x in t.tolist()]  # noqa: E731
        _, c, _ = _keyeddiff.keyed_diff(hexes[0], hexes[1], rows(host[1]), rows(host[3]))
        t1 = time.perf_counter()
        got = (c[_keyeddiff.ADDED], c[_keyeddiff.REMOVED], c[_keyeddiff.MODIFIED], c[_keyeddiff.UNCHANGED])
        how = "dict restatement"
    t2 = time.perf_counter()
    if got != (d.added, d.removed, d.modified, d.unchanged):
        sys.exit(f"keyed_diff_probe: the CPU join counts {got}, the device {d[3:7]}")
    return {"nleft": n, "nright": len(hexes[1]), "how": how, "join_s": round(t1 - t0, 3), "join_and_status_s": round(t2 - t0, 3),
            "added": got[0], "removed": got[1], "modified": got[2], "unchanged": got[3]}


if __name__ == "__main__":
    main()
