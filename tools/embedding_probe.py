"""The embedding query (oxh_embedding_*_device) at the sizes of a real table:
  similarity   1 M x 768 (3.07 GB) and 10 M x 64 float32, fixed layout, no validity: sim alone;
  ordered      the same with order_key + perm (the stable sort of the keys on top);
  mean         nidx = 1 and 100 000 of the 1 M x 768 column;
  chain        filter (`id == v`), mean, similarity, sort, the page of 100 rows: the whole device chain.
Beside the similarity, in the same run and alternating with it: `torch.mv(X, q)` on the same tensor, which reads
the same bytes once. The ratio goes into the JSON; none is fixed in advance. All inputs device-resident, HIP events
on the call's stream around the blocking call (and the host clock), two warm calls, medians of --reps. Every case
is checked on a sample of rows against float64 numpy (|sim - exact| <= (2 dim + 8) 2^-24), the order against the
returned keys. Which launch takes the time is a matter for
`rocprofv3 --kernel-trace --stats -- python tools/embedding_probe.py --reps 3`, in a run of its own.

    python tools/embedding_probe.py [--reps 15] [--shapes 1000000x768,10000000x64] [--out profiles/embedding/probe.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--shapes", default="1000000x768,10000000x64")
    ap.add_argument("--mean-nidx", default="1,100000")
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embedding", "probe.json"))
    a = ap.parse_args()

    import torch

    import _embedding as E
    from oxen_amd import _capi, tabular
    from oxen_amd.tabular import Column, Embedding

    if not torch.cuda.is_available():
        sys.exit("embedding_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    ctx = _capi.Context(0)
    stream = torch.cuda.Stream()
    torch.manual_seed(a.seed)

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
            sys.exit(f"embedding_probe: {what}")

    def alternating(mine, beside=None):
        for _ in range(2):
            mine()
            if beside:
                timed(beside)
        m, o = [], []
        for _ in range(a.reps):
            m.append(timed(mine))
            if beside:
                o.append(timed(beside))
        return m, o

    def check_similarity(name, x, q, got, n, dim):
        rows = torch.unique(torch.randint(0, n, (a.sample,), device=dev))
        xs, qd = x[rows].cpu().numpy().astype(np.float64), q.cpu().numpy().astype(np.float64)
        exact = (xs @ qd) / np.sqrt((xs * xs).sum(axis=1) * (qd * qd).sum())
        worst = float(np.abs(got.sim[rows].cpu().numpy().astype(np.float64) - exact).max())
        need(worst <= (2 * dim + 8) * 2.0 ** -24, f"{name}: a sample of rows is {worst:.3e} from float64")
        if got.perm is not None:
            key = got.order_key.cpu().numpy().view(np.uint32)
            bits = got.sim.cpu().numpy().view(np.uint32)
            sample = rows.cpu().numpy()
            need(all(int(key[r]) == E.order_key(int(bits[r])) for r in sample[:500]), f"{name}: a key is not its similarity's")
            perm = got.perm.cpu().numpy().view(np.uint32)
            ordered = key[perm].astype(np.int64)
            need(bool((np.diff(ordered) >= 0).all()), f"{name}: the keys do not ascend along perm")
            ties = np.diff(ordered) == 0
            need(bool((np.diff(perm.astype(np.int64))[ties] > 0).all()), f"{name}: tied rows are not in input order")
            need(np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), f"{name}: perm is no permutation")
        return worst

    result = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for shape in a.shapes.split(","):
        n, dim = (int(v) for v in shape.split("x"))
        x = torch.randn((n, dim), dtype=torch.float32, device=dev)
        q = torch.randn(dim, dtype=torch.float32, device=dev)
        emb = Embedding(_capi.OXH_EMB_FIXED, dim, n, x.reshape(-1))
        nbytes = 4 * n * dim
        torch.cuda.synchronize()
        cases = {}

        def call(order):
            return tabular.cosine_similarity_device(emb, q, want_order=order, stream=stream.cuda_stream, ctx=ctx)

        mine, other = alternating(lambda: call(False), lambda: torch.mv(x, q))
        m, o = stats(mine), stats(other)
        worst = check_similarity(f"{shape} similarity", x, q, mine[-1][2], n, dim)
        cases["similarity"] = {**m, "bytes_read": nbytes, "tb_per_s": round(nbytes / (m["event_ms_median"] * 1e-3) / 1e12, 3),
                               "torch_mv": {**o, "tb_per_s": round(nbytes / (o["event_ms_median"] * 1e-3) / 1e12, 3)},
                               "over_torch_mv": round(m["event_ms_median"] / o["event_ms_median"], 2), "worst_abs_error_sampled": worst}
        print(shape, "similarity", json.dumps(cases["similarity"]), flush=True)

        mine, _ = alternating(lambda: call(True))
        mo = stats(mine)
        check_similarity(f"{shape} ordered", x, q, mine[-1][2], n, dim)
        cases["ordered"] = {**mo, "added_ms_over_similarity": round(mo["event_ms_median"] - m["event_ms_median"], 4)}
        print(shape, "ordered", json.dumps(cases["ordered"]), flush=True)

        if dim >= 256:   # the mean and the chain on the wide column
            for nidx in (int(v) for v in a.mean_nidx.split(",")):
                idx = torch.sort(torch.randperm(n, device=dev)[:nidx])[0].to(torch.int32)
                mine, _ = alternating(lambda: tabular.embedding_mean_device(emb, idx, stream=stream.cuda_stream, ctx=ctx))
                mean, st = mine[-1][2]
                exact = x[idx.to(torch.int64)].to(torch.float64).mean(dim=0)
                err = float((mean.to(torch.float64) - exact).abs().max())
                need(st.used == nidx and err <= 1e-4, f"{shape} mean {nidx}: {st}, {err:.3e} from float64")
                again = tabular.embedding_mean_device(emb, idx, stream=stream.cuda_stream, ctx=ctx)[0]
                need(bool((again.view(torch.int32) == mean.view(torch.int32)).all()), f"{shape} mean {nidx}: two runs differ")
                cases[f"mean_{nidx}"] = {**stats(mine), "bytes_read": 4 * nidx * dim, "worst_abs_error": err}
                print(shape, f"mean_{nidx}", json.dumps(cases[f"mean_{nidx}"]), flush=True)
            ids = torch.arange(n, dtype=torch.int64, device=dev)
            frame = {"id": Column(8, n, ids)}
            where = f"id == {n // 3}"
            mine, _ = alternating(lambda: tabular.sort_by_similarity_device(frame, emb, where, 100, 1, stream=stream.cuda_stream, ctx=ctx))
            page = mine[-1][2]
            need(int(page["id"].values[0]) == n // 3 and page["embedding"].nrows == 100, f"{shape} chain: the page does not start with the query's row")
            need(bool((page["embedding"].values[:dim] == x[n // 3]).all()), f"{shape} chain: the page's first vector is not the row's")
            cases["chain_page_100"] = stats(mine)
            print(shape, "chain_page_100", json.dumps(cases["chain_page_100"]), flush=True)
        result["shapes"][shape] = {"rows": n, "dim": dim, **cases}
        del x, emb
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
