"""The batched Zstandard inflate (oxh_zstd_inflate_*) and the Parquet open that uses it, at the size of a real table:
tools/snappy_probe.py's input -- --rows (10 M) rows of tools/csv_probe.py's five-column shape, the uncompressed Parquet
bytes cut into 1 MiB pieces -- with every piece a Zstandard frame of pyarrow's codec at levels 1 and 3. Needs pyarrow
for the compressor (without it the probe says so and measures nothing: pre-compressed pieces are not kept anywhere).
It records, and fixes nothing in advance:
  frames   `zstd_inflate_device` over all frames of a level in one call; `pa.Codec("zstd").decompress` over the same
           frames on 16 threads; `snappy_inflate_device` over the Snappy twin of the same pieces; one `torch`
           device-to-device copy of the inflated bytes (the floor) -- alternated in one loop; then the same over
           incompressible pieces (Raw blocks) and constant ones (RLE blocks);
  open     `ParquetFile` on pyarrow's ZSTD file of the table beside its SNAPPY and uncompressed twins, on the device.
Two warm calls, medians of --reps, a host clock around calls that block until the device is done.

    python tools/zstd_inflate_probe.py [--rows 10000000] [--reps 5] [--out profiles/zstd/probe.json]
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


def frame_times(tabular, torch, pa, ctx, plain: bytes, reps: int, levels) -> dict:
    pieces = [plain[k:k + PIECE] for k in range(0, len(plain), PIECE)]
    up = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    offsets = lambda parts: up(np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64))  # noqa: E731
    d_do = offsets(pieces)
    d_dst, d_status = torch.empty(len(plain), dtype=torch.uint8, device="cuda:0"), torch.empty(len(pieces), dtype=torch.int32, device="cuda:0")
    d_other = torch.empty_like(d_dst)
    pool = ThreadPoolExecutor(16)
    calls, sizes, host_frames = {}, {}, None
    for name, codec in [("zstd_level_%d" % k, pa.Codec("zstd", compression_level=k)) for k in levels] + [("snappy", pa.Codec("snappy"))]:
        streams = [codec.compress(p).to_pybytes() for p in pieces]
        d_src, d_so = up(np.frombuffer(b"".join(streams), dtype=np.uint8).copy()), offsets(streams)
        entry = tabular.snappy_inflate_device if name == "snappy" else tabular.zstd_inflate_device

        def inflate(entry=entry, d_src=d_src, d_so=d_so):
            assert entry(d_src, d_so, d_dst, d_do, d_status, ctx=ctx, stream=ctx.stream) == 0

        d_dst.zero_()
        inflate()
        assert d_dst.cpu().numpy().tobytes() == plain, name
        calls[name + "_inflate_device"], sizes[name + "_bytes"] = inflate, int(d_src.numel())
        if name == "zstd_level_%d" % levels[-1]:
            host_frames, host_codec = streams, codec

    def floor():
        d_other.copy_(d_dst)
        torch.cuda.synchronize()

    def host():
        list(pool.map(lambda bp: host_codec.decompress(bp[0], decompressed_size=len(bp[1])), zip(host_frames, pieces)))

    t = alternated({**calls, "copy_floor": floor, "pyarrow_zstd_decompress_16_threads": host}, reps)
    gbs = lambda ms: round(len(plain) / 1e9 / (ms / 1e3), 2)  # noqa: E731
    t.update({"pieces": len(pieces), "inflated_bytes": len(plain), **sizes, "gb_s_out": {k: gbs(v["median_ms"]) for k, v in t.items()}})
    pool.shutdown()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd", "probe.json"))
    a = ap.parse_args()

    import torch

    from oxen_amd import _capi, tabular

    if not torch.cuda.is_available():
        sys.exit("zstd_inflate_probe: no GPU (there is nothing to measure on a CPU)")
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq
    except ImportError:
        sys.exit("zstd_inflate_probe: no pyarrow, so no compressor and no pre-compressed pieces: nothing measured")
    pa.set_cpu_count(16)
    ctx = _capi.Context(0)
    data, rows = five_columns(np.random.default_rng(a.seed), a.rows)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    ours = tabular.write_parquet_device(tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream), ctx=ctx, stream=ctx.stream).cpu().numpy().tobytes()
    del d
    out = {"rows": rows, "reps": a.reps, "piece_bytes": PIECE, "streams": "pyarrow's Codec('zstd') at levels 1 and 3 over 1 MiB pieces of the uncompressed Parquet file"}

    def record(key, value):
        out[key] = value
        print(json.dumps({key: value}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:   # after every part: a run that is cut short keeps what it measured
            json.dump(out, fh, indent=1)
            fh.write("\n")

    record("table_frames", frame_times(tabular, torch, pa, ctx, ours, a.reps, (1, 3)))
    noise = np.random.default_rng(a.seed).integers(0, 256, 128 << 20, dtype=np.uint8).tobytes()
    record("incompressible_frames", frame_times(tabular, torch, pa, ctx, noise, a.reps, (3,)))
    record("constant_frames", frame_times(tabular, torch, pa, ctx, bytes(128 << 20), a.reps, (3,)))
    table = pq.read_table(io.BytesIO(ours))
    files = {}
    for name, codec in (("zstd", "zstd"), ("snappy", "snappy"), ("uncompressed", "none")):
        sink = io.BytesIO()
        pq.write_table(table, sink, compression=codec, use_dictionary=False)
        files[name] = torch.from_numpy(np.frombuffer(sink.getvalue(), dtype=np.uint8).copy()).to("cuda:0")

    def opened(d_file):
        return lambda: tabular.ParquetFile(d_file, ctx=ctx, device=True, stream=ctx.stream).close()

    times = alternated({name: opened(d_file) for name, d_file in files.items()}, a.reps)
    with tabular.ParquetFile(files["zstd"], ctx=ctx, device=True, stream=ctx.stream) as f:
        times.update({name + "_file_bytes": int(d_file.numel()) for name, d_file in files.items()})
        times["stats8_zstd"] = list(f.stats)
    record("open", times)


if __name__ == "__main__":
    main()
