"""The dedup index at C5's size: one insert of 13.1 M digests (100 GiB at 8 KiB chunks) into a fresh
index, timed with HIP events around oxh_dedup_index_insert_device, in three mixes -- all distinct, half
duplicates, all equal -- with the table sized for the rows (no growth) and from the default capacity
(one growth: allocate, re-insert everything). Beside each, the time numpy.unique takes on the same
keys on the host. Every run's distinct count is checked against numpy's.

    python tools/dedup_index_probe.py [--rows 13107200] [--reps 5] [--out profiles/dedup_index/probe.json]
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


def mixes(n: int, seed: int):
    rng = np.random.default_rng(seed)
    distinct = rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    half = distinct.copy()
    half[n - n // 2:] = half[rng.integers(0, n - n // 2, size=n // 2)]  # the second half repeats rows of the first
    half = half[rng.permutation(n)]
    equal = np.tile(distinct[:1], (n, 1))
    return {"all_distinct": distinct, "half_duplicates": half, "all_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100 * 2**30 // 8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_index", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, dedup

    if not torch.cuda.is_available():
        sys.exit("dedup_index_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    ctx = _capi.Context(0)
    L = _capi.lib()
    n = a.rows
    stream = torch.cuda.Stream()
    d_lens = torch.full((n,), 8192, dtype=torch.int64, device=dev)
    d_first = torch.empty(n, dtype=torch.int64, device=dev)
    stats = np.zeros(4, dtype=np.uint64)

    def one_insert(d_dig, capacity):
        """(ms between HIP events around the call, ms of the blocking call on the host clock, stats)."""
        with dedup.DedupIndex(ctx, capacity) as idx:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record(stream)
            _capi.check(L.oxh_dedup_index_insert_device(idx.handle, d_dig.data_ptr(), d_lens.data_ptr(), n, d_first.data_ptr(),
                                                        stats.ctypes.data_as(_capi._u64p), stream.cuda_stream),
                        "oxh_dedup_index_insert_device")
            end.record(stream)
            end.synchronize()
            return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3, [int(v) for v in stats]

    result = {"rows": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "key_bytes": 16 * n,
              "table_slots_sized": 1 << (2 * n - 1).bit_length(), "mixes": {}}
    for name, keys in mixes(n, a.seed).items():
        t0 = time.perf_counter()
        n_unique = len(np.unique(keys.view([("lo", "<u8"), ("hi", "<u8")]).reshape(-1)))
        unique_s = time.perf_counter() - t0
        d_dig = torch.from_numpy(keys.view(np.int64)).to(dev)
        row = {"distinct": n_unique, "numpy_unique_s": round(unique_s, 3)}
        for label, capacity in (("sized", n), ("grown_from_default", 0)):
            one_insert(d_dig, capacity)  # warm-up: code objects, the allocator
            ev, wall = [], []
            for _ in range(a.reps):
                e, w, s = one_insert(d_dig, capacity)
                if s[0] != n_unique or s[0] + s[2] != n or s[1] + s[3] != 8192 * n:
                    sys.exit(f"dedup_index_probe: {name}/{label}: stats {s}, numpy.unique counts {n_unique} of {n}")
                ev.append(e)
                wall.append(w)
            row[label] = {"event_ms_median": round(float(np.median(ev)), 3), "event_ms_min": round(min(ev), 3),
                          "event_ms_max": round(max(ev), 3), "call_ms_median": round(float(np.median(wall)), 3),
                          "rows_per_us": round(n / (float(np.median(ev)) * 1e3), 1)}
        result["mixes"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_dig
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
