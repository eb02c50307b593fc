"""What the Zstandard fixtures and tests share: the plain inputs, built by explicit integer arithmetic (a splitmix64 over
numpy uint64, no library RNG) so that they are the same bytes on every machine, and one call of either form with the
frames at odd addresses and guard bytes around the destinations. tests/golden/make_zstd.py compresses the plains once;
the manifest records each plain's length and crc32."""
import ctypes
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd")
GUARD = 0xA5
CAUSES = {"frame": 1, "header": 2, "input": 3, "block": 4, "literals": 5, "table": 6, "sequences": 7, "offset": 8, "overrun": 9,
          "truncated": 10, "range": 11}   # OXH_ZSTD_*


def splitmix(n: int, seed: int) -> np.ndarray:
    """n words of splitmix64 from `seed`."""
    with np.errstate(over="ignore"):
        x = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def random_bytes(n: int, seed: int) -> bytes:
    return splitmix((n + 7) // 8, seed).astype("<u8").tobytes()[:n]


def words(n: int, seed: int) -> bytes:
    """n bytes of text over 150 pseudo-words of 2 to 9 letters, the frequent ones first."""
    vocabulary = [bytes(97 + int(c) % 26 for c in splitmix(2 + k % 8, 1000 + k) >> np.uint64(40)) for k in range(150)]
    picks = (splitmix(n // 2 + 1, seed) >> np.uint64(33)) % np.uint64(150)
    picks = picks * ((splitmix(n // 2 + 1, seed + 1) >> np.uint64(33)) % np.uint64(150)) // np.uint64(150)   # skewed to the first
    return b" ".join(vocabulary[int(k)] for k in picks)[:n]


def skewed(n: int, seed: int, first: int = 65) -> bytes:
    """n bytes over the 5 symbols from `first` with probabilities 1/2, 1/4, 1/8, 1/16, 1/16."""
    r = (splitmix(n, seed) >> np.uint64(60)).astype(np.uint8)
    return (first + np.select([r < 8, r < 12, r < 14, r < 15], [0, 1, 2, 3], 4)).astype(np.uint8).tobytes()


def plains() -> dict:
    piece = random_bytes(35000, 7)
    return {
        "empty": b"", "one_byte": b"x", "constant_5000": b"\x07" * 5000, "constant_300000": b"z" * 300000,
        "random_1000": random_bytes(1000, 1), "random_132000": random_bytes(132000, 2),
        "words_200": words(200, 3), "words_900": words(900, 4), "words_5000": words(5000, 5), "words_150000": words(150000, 6), "words_400000": words(400000, 6),
        "period_7": b"abcdefg" * 700, "ramp_int64": np.arange(4000, dtype="<i8").tobytes(),
        "small_int64": ((splitmix(6000, 8) >> np.uint64(58)).astype("<i8")).tobytes(),
        "rounded_doubles": (((splitmix(6000, 9) >> np.uint64(50)).astype(np.float64) / 100.0).astype("<f8")).tobytes(),
        "skewed_5": skewed(60000, 10), "skewed_low": skewed(3000, 11, first=0), "piece_three_times": piece * 3,
    }


def manifest() -> dict:
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def frame(name: str) -> bytes:
    with open(os.path.join(GOLDEN, name + ".zst"), "rb") as f:
        return f.read()


def run(ctx, frames, wants, form):
    """(outputs, statuses, bad_blocks) of one call over the frames, back to back from an odd address, into destinations
    back to back from an odd address inside a buffer of guard bytes, which must stay as they were."""
    from oxen_amd import _capi, tabular

    n, lead = len(frames), 3
    src = np.frombuffer(b"\x55" * lead + b"".join(frames), dtype=np.uint8).copy()
    src_offsets = (lead + np.concatenate([[0], np.cumsum([len(b) for b in frames])])).astype(np.int64)
    dst_offsets = (5 + np.concatenate([[0], np.cumsum(wants)])).astype(np.int64)
    dst = np.full(int(dst_offsets[-1]) + 7, GUARD, dtype=np.uint8)
    status = np.full(n, 99, dtype=np.int32)
    if form == "host":
        bad = ctypes.c_uint64(99)
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)  # noqa: E731
        _capi.check(_capi.lib().oxh_zstd_inflate_host(ctx.handle, n, src.ctypes.data, u64(src_offsets), dst.ctypes.data, u64(dst_offsets),
                                                      status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(bad)), "oxh_zstd_inflate_host")
        bad = bad.value
    else:
        import torch

        up = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
        d_dst, d_status = up(dst), up(status)
        bad = tabular.zstd_inflate_device(up(src), up(src_offsets), d_dst, up(dst_offsets), d_status, ctx=ctx, stream=ctx.stream)
        dst, status = d_dst.cpu().numpy(), d_status.cpu().numpy()
    assert np.all(dst[:5] == GUARD) and np.all(dst[int(dst_offsets[-1]):] == GUARD), "a guard byte was written"
    raw = dst.tobytes()
    return [raw[int(dst_offsets[k]):int(dst_offsets[k + 1])] for k in range(n)], [int(s) for s in status], bad
