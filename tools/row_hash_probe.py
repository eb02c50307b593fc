"""Row hashes of a device-resident frame (oxh_row_hashes_device) and the row diff (oxh_row_diff_device) at
the size of a real table: --rows (10 M) rows of Int64, Float64, Boolean and two string columns of mean
24 B ("short"), and --long-rows rows of one string column of mean 2 KiB ("long"). Recorded, per frame:

  (a) fused     the call as shipped: length pass, one lane per short row through LDS, long rows through
                the arena and K1;
  (b) two_pass  the same rows gathered whole into an arena by the long-row kernel and hashed by the
                lane-per-item kernel (oxh_set_kernel_variant(9001): the two-pass form built from the same
                pieces); its digests must equal (a)'s;
  (c) cpu       the reference's loop restated on the CPU over the first --cpu-rows rows (at most 128 MiB of
                them): numpy row assembly by the row-bytes rule (one thread, vectorised), then the C oracle's
                XXH3-128 with 16 threads, as bench.py's CPU leg; the device digests are checked against it;
  (d) diff      oxh_row_diff_device of (a)'s digest table against a copy with 1 % of the rows changed,
                beside one oxh_dedup_index_insert_device of the same 2 x rows into a fresh index.

(a) and (b), and the two of (d), alternate in one process; one warm call each first; medians of --reps.
Times are HIP events around the blocking call and the host clock around it (the call allocates and reads
its control words back, so the host clock is the larger).

    python tools/row_hash_probe.py [--rows 10000000] [--long-rows 1000000] [--reps 5] [--out profiles/row_hash/probe.json]
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

GATHER_ALL = 9001  # row_hash.hip: every row through the arena, hashed by the lane kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--long-rows", type=int, default=1_000_000)
    ap.add_argument("--cpu-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_hash", "probe.json"))
    a = ap.parse_args()

    import torch

    from oracle import oracle
    from oxen_amd import _capi, dedup, tabular
    from oxen_amd.tabular import Column

    if not torch.cuda.is_available():
        sys.exit("row_hash_probe: no GPU (there is nothing to measure on a CPU)")
    oracle.build()
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

    def strings(n, top):
        lens = torch.randint(0, top + 1, (n,), dtype=torch.int64, device=dev)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        total = int(offsets[-1])
        values = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
        if total < 2**31:
            return Column(tabular.OXH_COL_BYTES32, n, values, offsets.to(torch.int32))
        return Column(tabular.OXH_COL_BYTES64, n, values, offsets)

    def frame(kind):
        if kind == "short":
            n = a.rows
            return [Column(8, n, torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device=dev)),
                    Column(8, n, torch.randn(n, dtype=torch.float64, device=dev)),
                    Column(tabular.OXH_COL_BOOL, n, torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev)),
                    strings(n, 48), strings(n, 48)]
        return [strings(a.long_rows, 4096)]

    def row_bytes(cols):
        return sum(int(c.offsets[-1]) - int(c.offsets[0]) if c.offsets is not None else c.nrows * (1 if c.kind == 16 else c.kind)
                   for c in cols)

    def cpu_leg(cols, n):
        """numpy assembly of the first n rows + the oracle's XXH3 with 16 threads; the digests."""
        host = []
        for c in cols:
            if c.offsets is not None:
                off = c.offsets[: n + 1].cpu().numpy().astype(np.int64)
                host.append((c.kind, off - off[0], c.values[int(off[0]):int(off[-1])].cpu().numpy()))
            elif c.kind == 16:
                host.append((16, None, np.unpackbits(c.values[: (n + 7) // 8].cpu().numpy(), bitorder="little")[:n]))
            else:
                host.append((c.kind, None, c.values[:n].cpu().numpy().view(np.uint8).reshape(n, c.kind)))
        t0 = time.perf_counter()
        lens = np.zeros(n, dtype=np.int64)
        for kind, off, _ in host:
            lens += (off[1:] - off[:-1]) if off is not None else (1 if kind == 16 else kind)
        starts = np.cumsum(lens) - lens
        arena = np.zeros(max(1, int(lens.sum())), dtype=np.uint8)
        at = starts.copy()
        for kind, off, data in host:
            if off is None:
                w = 1 if kind == 16 else kind
                arena[(at[:, None] + np.arange(w)).reshape(-1)] = data.reshape(-1)
                at += w
            else:
                cl = off[1:] - off[:-1]
                within = np.arange(int(cl.sum()), dtype=np.int64) - np.repeat(off[:-1], cl)
                arena[np.repeat(at, cl) + within] = data
                at += cl
        t1 = time.perf_counter()
        dig = oracle.batch(arena, starts.astype(np.uint64), lens.astype(np.uint64), threads=16)
        t2 = time.perf_counter()
        return dig, {"rows": n, "threads": 16, "assemble_s": round(t1 - t0, 4), "hash_s": round(t2 - t1, 4),
                     "rows_per_s": round(n / (t2 - t0))}

    result = {"rows": a.rows, "long_rows": a.long_rows, "reps": a.reps, "device": torch.cuda.get_device_name(0), "frames": {}}
    digests = None
    for kind in ("short", "long"):
        cols = frame(kind)
        n = cols[0].nrows
        torch.cuda.synchronize()

        def fused():
            return tabular.row_hashes_device(cols, stream=stream, ctx=ctx)

        def two_pass():
            L.oxh_set_kernel_variant(GATHER_ALL)
            try:
                return tabular.row_hashes_device(cols, stream=stream, ctx=ctx)
            finally:
                L.oxh_set_kernel_variant(0)

        want = fused()  # warm: code objects, the scratch lease
        if not torch.equal(two_pass(), want):
            sys.exit(f"row_hash_probe: {kind}: the two-pass digests differ from the fused call's")
        fu, tp = [], []
        for _ in range(a.reps):  # alternating
            fu.append(timed(fused))
            tp.append(timed(two_pass))
        nbytes = row_bytes(cols)
        cpu_n = min(n, a.cpu_rows, max(1000, int(2**27 // max(1.0, nbytes / n))))  # at most 128 MiB of rows on the host
        cpu_dig, cpu = cpu_leg(cols, cpu_n)
        if not np.array_equal(cpu_dig, want[:cpu_n].cpu().numpy().view(np.uint64)):
            sys.exit(f"row_hash_probe: {kind}: the device digests differ from the CPU restatement's")
        row = {"rows": n, "columns": len(cols), "row_bytes_total": nbytes, "row_bytes_mean": round(nbytes / n, 1),
               "fused_event_ms_median": med(fu, 0), "fused_event_ms_min": round(min(x[0] for x in fu), 3),
               "fused_call_ms_median": med(fu, 1),
               "two_pass_event_ms_median": med(tp, 0), "two_pass_event_ms_min": round(min(x[0] for x in tp), 3),
               "two_pass_call_ms_median": med(tp, 1),
               "fused_rows_per_s": round(n / (med(fu, 1) * 1e-3)), "fused_gb_per_s": round(nbytes / (med(fu, 1) * 1e-3) / 1e9, 1),
               "two_pass_over_fused": round(med(tp, 1) / med(fu, 1), 2), "cpu": cpu, "digests_checked_against_cpu": cpu_n}
        result["frames"][kind] = row
        print(kind, json.dumps(row), flush=True)
        if kind == "short":
            digests = want
        del cols

    # (d) the diff of two digest tables beside one index insert of the same rows
    n = digests.shape[0]
    head = digests.clone()
    changed = torch.rand(n, device=dev) < 0.01
    head[changed] = torch.randint(-(1 << 63), (1 << 63) - 1, (int(changed.sum()), 2), dtype=torch.int64, device=dev)
    both = torch.cat([digests, head])
    d_first = torch.empty(2 * n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def diff():
        return tabular.row_diff_device(digests, head, stream=stream, ctx=ctx)

    def insert():
        with dedup.DedupIndex(ctx, 2 * n) as idx:
            return timed(lambda: _capi.check(
                L.oxh_dedup_index_insert_device(idx.handle, both.data_ptr(), None, 2 * n, d_first.data_ptr(), None,
                                                stream.cuda_stream), "oxh_dedup_index_insert_device"))

    _, _, counts = diff()
    if counts != (int(changed.sum()), int(changed.sum())):
        sys.exit(f"row_hash_probe: the diff reports {counts}, {int(changed.sum())} rows were changed")
    insert()
    df, ins = [], []
    for _ in range(a.reps):
        df.append(timed(diff))
        ins.append(insert())
    result["diff"] = {"rows_each": n, "changed": int(changed.sum()), "diff_event_ms_median": med(df, 0),
                      "diff_call_ms_median": med(df, 1), "insert_event_ms_median": med(ins, 0),
                      "insert_call_ms_median": med(ins, 1), "diff_over_insert": round(med(df, 1) / med(ins, 1), 2)}
    print("diff", json.dumps(result["diff"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
