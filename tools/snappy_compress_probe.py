"""The batched Snappy compress (oxh_snappy_compress_*) at the size of a real table: --rows (10 M) rows of
tools/csv_probe.py's five-column shape, written as an uncompressed Parquet file and cut into 1 MiB pieces -- what a
file of 1 MiB pages would compress. Needs pyarrow for the codec it is compared with (without it the probe says so and
measures nothing). For the table's pieces, for incompressible pieces and for constant pieces it records, and fixes
nothing in advance: `snappy_compress_device` over all pieces in one call with the GB/s of input, the compressed size
beside `pa.Codec("snappy")`'s on the same pieces and their ratio, that codec's time on 16 threads, and one `torch`
device-to-device copy of the input (the floor) -- all alternated in one loop, so they see the same machine; then the
Parquet write of the table with and without OXH_PARQUET_SNAPPY, in the device and the host form. Every
stream is inflated again by `snappy_inflate_device` and compared with its piece before anything is timed.
The table's size and the stride over barren batches are chosen from the `arms` it records: the shipped library and, each
in a process of its own, libraries built from snappy_compress.hip with OXH_SNAPPY_TABLE_BITS / OXH_SNAPPY_WIDEN.
Two warm calls, medians of --reps, a host clock around calls that block until the device is done.

    python tools/snappy_compress_probe.py [--rows 10000000] [--reps 5] [--out profiles/snappy_compress/probe.json]
"""
from __future__ import annotations

import argparse
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
# (log2 of the table's entries, widening stride over barren batches): the arms the two parameters are chosen from.
# The first is what the library ships; the others are built here from snappy_compress.hip with the two defines.
ARMS = ((12, 1), (12, 0), (13, 0), (14, 0), (13, 1))


def build_arm(bits: int, widen: int) -> str:
    """The library with snappy_compress.hip rebuilt for one arm (the other objects are the main build's)."""
    import subprocess

    from oxen_amd import build

    out = os.path.join(build.HERE, "build", "arms", "liboxen_hash_t%d_w%d.so" % (bits, widen))
    src = os.path.join(build.CSRC, "snappy_compress.hip")
    if os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(src):
        return out
    objdir = os.path.join(build.HERE, "build", "liboxen_hash")
    objs = [os.path.join(objdir, os.path.basename(f) + ".o") for f in build.SOURCES]
    if not all(os.path.exists(o) for o in objs):
        build.compile_lib(build.LIB)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    mine = out[:-3] + ".o"
    subprocess.run([build.hipcc(), "--offload-arch=" + build.ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Xclang", "-target-feature", "-Xclang",
                    "-packed-fp32-ops", "-DOXH_SNAPPY_TABLE_BITS=%d" % bits, "-DOXH_SNAPPY_WIDEN=%d" % widen, "-c", "-o", mine, src], check=True)
    subprocess.run([build.hipcc(), "--offload-arch=" + build.ARCH, "-shared", "-fPIC", "-Wl,--no-undefined", "-o", out] +
                   [mine if o.endswith("snappy_compress.hip.o") else o for o in objs], check=True)
    return out


def piece_times(tabular, torch, pa, ctx, plain: bytes, reps: int) -> dict:
    codec = pa.Codec("snappy")
    pieces = [plain[k:k + PIECE] for k in range(0, len(plain), PIECE)]
    up = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    offsets = lambda sizes: up(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))  # noqa: E731
    d_src, d_so = up(np.frombuffer(plain, dtype=np.uint8).copy()), offsets([len(p) for p in pieces])
    d_do = offsets([tabular.snappy_bound(len(p)) for p in pieces])
    d_dst = torch.empty(int(d_do[-1]), dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.empty(len(pieces), dtype=torch.int64, device="cuda:0")
    d_status = torch.empty(len(pieces), dtype=torch.int32, device="cuda:0")
    d_other = torch.empty_like(d_src)
    pool = ThreadPoolExecutor(16)

    def compress():
        tabular.snappy_compress_device(d_src, d_so, d_dst, d_do, d_sizes, d_status, ctx=ctx, stream=ctx.stream)

    def floor():
        d_other.copy_(d_src)
        torch.cuda.synchronize()

    def host():
        return list(pool.map(codec.compress, pieces))

    compress()
    assert not d_status.any().item()
    # the streams, gathered back to back, inflate to the pieces
    sizes, lo = d_sizes.cpu().numpy(), d_do.cpu().numpy()
    d_packed = torch.cat([d_dst[int(a):int(a) + int(s)] for a, s in zip(lo, sizes)])
    d_back, d_bad = torch.empty_like(d_src), torch.empty(len(pieces), dtype=torch.int32, device="cuda:0")
    assert tabular.snappy_inflate_device(d_packed, offsets(sizes), d_back, d_so, d_bad, ctx=ctx, stream=ctx.stream) == 0
    assert torch.equal(d_back, d_src)
    del d_packed, d_back
    theirs = sum(len(b) for b in host())
    t = alternated({"compress_device": compress, "copy_floor": floor, "pyarrow_compress_16_threads": host}, reps)
    gbs = lambda ms: round(len(plain) / 1e9 / (ms / 1e3), 2)  # noqa: E731
    t.update({"pieces": len(pieces), "input_bytes": len(plain), "compressed_bytes": int(sizes.sum()), "pyarrow_compressed_bytes": theirs,
              "size_over_pyarrow": round(float(sizes.sum()) / theirs, 4), "compress_gb_s_in": gbs(t["compress_device"]["median_ms"]),
              "floor_gb_s_one_way": gbs(t["copy_floor"]["median_ms"]), "pyarrow_gb_s_in": gbs(t["pyarrow_compress_16_threads"]["median_ms"])})
    pool.shutdown()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snappy_compress", "probe.json"))
    ap.add_argument("--build-arms", action="store_true", help="only build the arms' libraries (needs no GPU)")
    ap.add_argument("--arm-lib", help="a child of this probe: the pieces' measurements with this library, as one JSON line")
    a = ap.parse_args()
    if a.build_arms:
        print([build_arm(*arm) for arm in ARMS[1:]])
        return

    import torch

    from oxen_amd import _capi, tabular

    if not torch.cuda.is_available():
        sys.exit("snappy_compress_probe: no GPU (there is nothing to measure on a CPU)")
    try:
        import pyarrow as pa
    except ImportError:
        sys.exit("snappy_compress_probe: no pyarrow, so no codec to compare with: nothing measured")
    pa.set_cpu_count(16)
    if a.arm_lib:
        _capi.LIB_PATH = a.arm_lib
    ctx = _capi.Context(0)
    data, rows = five_columns(np.random.default_rng(a.seed), a.rows)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    d_frame = tabular.read_csv_device(d, ctx=ctx, stream=ctx.stream)
    ours = tabular.write_parquet_device(d_frame, ctx=ctx, stream=ctx.stream).cpu().numpy().tobytes()
    del d
    out = {"rows": rows, "reps": a.reps, "piece_bytes": PIECE}
    inputs = {"table_pieces": ours, "incompressible_pieces": np.random.default_rng(a.seed).integers(0, 256, 256 << 20, dtype=np.uint8).tobytes(),
              "constant_pieces": bytes([7]) * (256 << 20)}
    for name, plain in inputs.items():
        if a.arm_lib and name == "constant_pieces":
            continue
        out[name] = piece_times(tabular, torch, pa, ctx, plain, a.reps)
        print(name, json.dumps(out[name]), flush=True)
    if a.arm_lib:
        print("ARM " + json.dumps({k: out[k] for k in ("table_pieces", "incompressible_pieces")}), flush=True)
        return
    # the arms: the shipped library's numbers above, every other arm in a process of its own with its own library
    import subprocess

    brief = lambda r: {k: {f: t[f] for f in ("compress_device", "compressed_bytes", "size_over_pyarrow", "compress_gb_s_in")}  # noqa: E731
                       for k, t in r.items() if k in ("table_pieces", "incompressible_pieces")}
    out["arms"] = {"table_bits_%d_widen_%d" % ARMS[0]: dict(brief(out), shipped=True)}
    for arm in ARMS[1:]:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--reps", str(a.reps), "--seed", str(a.seed),
                              "--arm-lib", build_arm(*arm)], capture_output=True, text=True, timeout=600)
        line = [x for x in run.stdout.splitlines() if x.startswith("ARM ")]
        out["arms"]["table_bits_%d_widen_%d" % arm] = brief(json.loads(line[0][4:])) if run.returncode == 0 and line else {"failed": run.stderr[-400:]}
        print(arm, json.dumps(out["arms"]["table_bits_%d_widen_%d" % arm]), flush=True)
    # the Parquet write with and without OXH_PARQUET_SNAPPY, in both forms (the Python entries: measure, allocate, write)
    h_frame = tabular.read_parquet(ours, ctx=ctx)
    writes = {"device_uncompressed": lambda: tabular.write_parquet_device(d_frame, ctx=ctx, stream=ctx.stream),
              "device_snappy": lambda: tabular.write_parquet_device(d_frame, ctx=ctx, stream=ctx.stream, compression="snappy"),
              "host_uncompressed": lambda: tabular.write_parquet(h_frame, ctx=ctx),
              "host_snappy": lambda: tabular.write_parquet(h_frame, ctx=ctx, compression="snappy")}
    out["parquet_write"] = alternated(writes, a.reps)
    out["parquet_write"].update({"uncompressed_file_bytes": len(ours), "snappy_file_bytes": len(writes["host_snappy"]())})
    print("parquet_write", json.dumps(out["parquet_write"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
