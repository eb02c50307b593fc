"""Chunk overlap at C5's size: oxh_chunk_overlap_device over 13.1 M digests (100 GiB at 8 KiB chunks)
cut into 2 sets (one mask word per row) and into 16, and over 200 sets of 65 536 rows (four words), in
three mixes -- all distinct, each set sharing half its rows with the one before, all equal -- timed with
HIP events around the call, one warm call first, median of --reps. The yardstick, in the same process
and alternating with it: oxh_dedup_index_insert_device of the same rows into a fresh index sized for
them (the overlap call makes and frees such an index itself, so its time holds the allocations the
yardstick's does not: `call_ms` is the host clock around the blocking call). Every matrix is checked
against what the mix was built to give. Host baselines: a Python set-membership loop at 1 M rows, and
the reference's list-contains loop (oxendedup.rs:56-70) at 20 000 x 20 000 rows only -- it is quadratic.

    python tools/chunk_overlap_probe.py [--rows 13107200] [--reps 5] [--out profiles/chunk_overlap/probe.json]
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


def host_baselines(seed: int) -> dict:
    rng = np.random.default_rng(seed)
    out = {}
    for label, n in (("python_set_loop", 1_000_000), ("reference_list_contains_loop", 20_000)):
        a = [str(v) for v in rng.integers(0, 1 << 62, size=n)]
        b = a[: n // 2] + [str(v) for v in rng.integers(0, 1 << 62, size=n - n // 2)]
        t0 = time.perf_counter()
        if label == "python_set_loop":
            members = set(b)
            overlap = sum(1 for h in a if h in members)
        else:
            overlap = sum(1 for h in a if h in b)  # Vec::contains: a scan per hash
        out[label] = {"rows_each": n, "seconds": round(time.perf_counter() - t0, 3), "overlap": overlap}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100 * 2**30 // 8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host baselines (a profiling pass)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_overlap", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, dedup

    if not torch.cuda.is_available():
        sys.exit("chunk_overlap_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    ctx = _capi.Context(0)
    L = _capi.lib()
    stream = torch.cuda.Stream()
    torch.manual_seed(a.seed)
    shapes = [("2_sets", [a.rows - a.rows // 2, a.rows // 2]), ("16_sets", [a.rows // 16] * 16),
              ("200_sets_of_65536", [65536] * 200)]
    result = {"rows": a.rows, "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record(stream)
        fn()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3

    for shape, sizes in shapes:
        n, nsets = sum(sizes), len(sizes)
        first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        d_lens = torch.full((n,), 8192, dtype=torch.int64, device=dev)
        d_first = torch.empty(n, dtype=torch.int64, device=dev)
        rows_out = np.zeros((nsets, nsets), dtype=np.uint64)
        bytes_out = np.zeros((nsets, nsets), dtype=np.uint64)
        stats = np.zeros(4, dtype=np.uint64)
        result["shapes"][shape] = {"rows": n, "nsets": nsets, "mask_words": (nsets + 63) // 64, "mixes": {}}
        for mix in ("all_distinct", "half_shared", "all_equal"):
            d_dig = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), dtype=torch.int64, device=dev)
            want = np.diag(np.array(sizes, dtype=np.uint64))
            if mix == "half_shared":  # the first half of set k = the second (fresh) half of set k-1, in random order
                for k in range(1, nsets):
                    h = min(sizes[k], sizes[k - 1]) // 2
                    b = int(first[k])  # where set k begins and set k-1 ends
                    d_dig[b:b + h] = d_dig[b - h:b][torch.randperm(h, device=dev)]
                    want[k, k - 1] = want[k - 1, k] = h
            elif mix == "all_equal":
                d_dig[:] = d_dig[0].clone()
                want = np.repeat(np.array(sizes, dtype=np.uint64)[:, None], nsets, axis=1)
            torch.cuda.synchronize()

            def overlap():
                _capi.check(L.oxh_chunk_overlap_device(ctx.handle, d_dig.data_ptr(), d_lens.data_ptr(),
                                                       first.ctypes.data_as(_capi._u64p), nsets,
                                                       rows_out.ctypes.data_as(_capi._u64p),
                                                       bytes_out.ctypes.data_as(_capi._u64p), stream.cuda_stream),
                            "oxh_chunk_overlap_device")

            def verify():
                if not (np.array_equal(rows_out, want) and np.array_equal(bytes_out, want * np.uint64(8192))):
                    sys.exit(f"chunk_overlap_probe: {shape}/{mix}: the matrix is not what the mix was built to give")
                rows_out[:] = 0
                bytes_out[:] = 0

            def insert():
                with dedup.DedupIndex(ctx, n) as idx:
                    t = timed(lambda: _capi.check(
                        L.oxh_dedup_index_insert_device(idx.handle, d_dig.data_ptr(), d_lens.data_ptr(), n, d_first.data_ptr(),
                                                        stats.ctypes.data_as(_capi._u64p), stream.cuda_stream),
                        "oxh_dedup_index_insert_device"))
                return t

            overlap()  # warm: code objects, the allocator
            verify()
            insert()
            ov, ins = [], []
            for _ in range(a.reps):  # alternating
                ov.append(timed(overlap))
                verify()
                ins.append(insert())
            med = lambda xs, k: round(float(np.median([x[k] for x in xs])), 3)
            row = {"overlap_event_ms_median": med(ov, 0), "overlap_event_ms_min": round(min(x[0] for x in ov), 3),
                   "overlap_event_ms_max": round(max(x[0] for x in ov), 3), "overlap_call_ms_median": med(ov, 1),
                   "insert_event_ms_median": med(ins, 0), "insert_call_ms_median": med(ins, 1),
                   "overlap_over_insert": round(med(ov, 0) / med(ins, 0), 2)}
            result["shapes"][shape]["mixes"][mix] = row
            print(shape, mix, json.dumps(row), flush=True)
            del d_dig
        del d_lens, d_first
    if not a.no_host:
        result["host"] = host_baselines(a.seed)
        print("host", json.dumps(result["host"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
