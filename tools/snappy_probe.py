"""The batched Snappy inflate (oxh_snappy_inflate_*) and the Parquet open that uses it, at the size of a real table:
--rows (10 M) rows of tools/csv_probe.py's five-column shape. Needs pyarrow for the compressor (without it the probe
says so and measures nothing: there is no compressor here). It records, and fixes nothing in advance:
  blocks   the table's uncompressed Parquet bytes cut into 1 MiB pieces, each a raw Snappy block of pyarrow's codec --
           what a file of 1 MiB pages holds: `snappy_inflate_device` over all blocks in one call, one `torch`
           device-to-device copy of the inflated bytes (the floor), `pa.Codec.decompress` over the same blocks on 16
           threads, and the same three over incompressible pieces (one long literal each: the copy-rate case) -- all
           alternated in one loop, so they see the same machine;
  open     `ParquetFile` on pyarrow's SNAPPY file of the table and on its uncompressed twin, both on the device.
Two warm calls, medians of --reps, a host clock around calls that block until the device is done.

    python tools/snappy_probe.py [--rows 10000000] [--reps 5] [--out profiles/snappy/probe.json]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from csv_probe import five_columns  # noqa: E402
from json_write_probe import alternated  # noqa: E402

PIECE = 1 << 20


def block_times(tabular, torch, pa, ctx, plain: bytes, reps: int) -> dict:
    codec = pa.Codec("snappy")
    pieces = [plain[k:k + PIECE] for k in range(0, len(plain), PIECE)]
    blocks = [codec.compress(p).to_pybytes() for p in pieces]
    up = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    offsets = lambda parts: up(np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64))  # noqa: E731
    d_src, d_so, d_do = up(np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()), offsets(blocks), offsets(pieces)
    d_dst, d_status = torch.empty(len(plain), dtype=torch.uint8, device="cuda:0"), torch.empty(len(blocks), dtype=torch.int32, device="cuda:0")
    d_other = torch.empty_like(d_dst)
    pool = ThreadPoolExecutor(16)

    def inflate():
        assert tabular.snappy_inflate_device(d_src, d_so, d_dst, d_do, d_status, ctx=ctx, stream=ctx.stream) == 0

    def floor():
        d_other.copy_(d_dst)
        torch.cuda.synchronize()

    def host():
        list(pool.map(lambda bp: codec.decompress(bp[0], decompressed_size=len(bp[1])), zip(blocks, pieces)))

    inflate()
    assert d_dst.cpu().numpy().tobytes() == plain
    t = alternated({"inflate_device": inflate, "copy_floor": floor, "pyarrow_decompress_16_threads": host}, reps)
    gbs = lambda ms: round(len(plain) / 1e9 / (ms / 1e3), 2)  # noqa: E731
    t.update({"blocks": len(blocks), "compressed_bytes": int(d_src.numel()), "inflated_bytes": len(plain),
              "inflate_gb_s_out": gbs(t["inflate_device"]["median_ms"]), "floor_gb_s_one_way": gbs(t["copy_floor"]["median_ms"]),
              "pyarrow_gb_s_out": gbs(t["pyarrow_decompress_16_threads"]["median_ms"])})
    pool.shutdown()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snappy", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular

    if not torch.cuda.is_available():
        sys.exit("snappy_probe: no GPU (there is nothing to measure on a CPU)")
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq
    except ImportError:
        sys.exit("snappy_probe: no pyarrow, so no compressor: nothing measured")
    pa.set_cpu_count(16)
    ctx = _capi.Context(0)
    data, rows = five_columns(np.random.default_rng(a.seed), a.rows)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    ours = tabular.write_parquet_device(tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream), ctx=ctx, stream=ctx.stream).cpu().numpy().tobytes()
    del d
    out = {"rows": rows, "reps": a.reps, "piece_bytes": PIECE, "streams": "pyarrow's Codec('snappy') over 1 MiB pieces of the uncompressed Parquet file",
           "table_blocks": block_times(tabular, torch, pa, ctx, ours, a.reps)}
    print(json.dumps(out["table_blocks"]), flush=True)
    noise = np.random.default_rng(a.seed).integers(0, 256, 256 << 20, dtype=np.uint8).tobytes()
    out["all_literal_blocks"] = block_times(tabular, torch, pa, ctx, noise, a.reps)
    print(json.dumps(out["all_literal_blocks"]), flush=True)
    table = pq.read_table(io.BytesIO(ours))
    files = {}
    for name, codec in (("snappy", "snappy"), ("uncompressed", "none")):
        sink = io.BytesIO()
        pq.write_table(table, sink, compression=codec, use_dictionary=False)
        files[name] = torch.from_numpy(np.frombuffer(sink.getvalue(), dtype=np.uint8).copy()).to("cuda:0")

    def opened(d_file):
        return lambda: tabular.ParquetFile(d_file, ctx=ctx, device=True, stream=ctx.stream).close()

    out["open"] = alternated({name: opened(d_file) for name, d_file in files.items()}, a.reps)
    with tabular.ParquetFile(files["snappy"], ctx=ctx, device=True, stream=ctx.stream) as f:
        out["open"].update({"snappy_file_bytes": int(files["snappy"].numel()), "uncompressed_file_bytes": int(files["uncompressed"].numel()),
                            "stats8_snappy": list(f.stats)})
    print(json.dumps(out["open"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
