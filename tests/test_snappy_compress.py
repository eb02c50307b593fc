"""The batched Snappy compress on the GPU (oxh_snappy_compress_*, oxen_amd/csrc/snappy_compress.hip) against the plain
byte-by-byte decoder of tests/_snappy_cases.py: every stream inflates to its input and stays inside the bound, at the
edges of a match, a 16-byte store, a batch of 64 positions and the 64 KiB fragment cut; size conditions that follow
from the format; placement, refused ranges and more blocks than the grid; determinism; pyarrow's decoder where it
imports."""
import ctypes

import numpy as np
import pytest

import _parquet_cases as K
import _snappy_cases as S
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
FORMS = ["host", "device"]
RANGE = 7   # OXH_SNAPPY_RANGE


def pat(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def period(p, n):
    return (pat(p, p) * (n // p + 1))[:n]


def ends(total, t):   # a 50-byte match that ends t bytes in front of the last byte of a block of `total` bytes
    base = pat(total - 50 - t, 5)
    return base + base[:50] + pat(t, 9)


CASES = {**{"mixed_%d" % n: (b"abcdefgh" * 9000)[:n] for n in (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 65535, 65536, 65537, 131073)},
         **{"random_%d" % n: pat(n) for n in (60, 61, 256, 257, 65536)},
         **{"period_%d" % p: period(p, 3 * p + 200) for p in (1, 2, 3, 7, 63, 64, 65, 2047, 2048, 2049)},
         "period_65535": period(65535, 65536),
         "period_65536": pat(65536) * 2,   # two fragments: the match would cross the cut
         **{"match_ends_%d_before_the_fragments_end" % t: ends(65536, t) + b"tail of the next fragment" for t in range(4)},
         **{"match_ends_%d_before_the_blocks_end" % t: ends(300, t) for t in range(4)},
         "run_of_100000": bytes([7]) * 100000,
         "text": "".join(K.cells(K.ROWS)["u"]).encode() * 8}


def run(ctx, blocks, form, fill=S.GUARD, room=None):
    """(streams, sizes, statuses) of one call: the blocks back to back from an odd address; destination range b has
    room[b] bytes (the bound where not given), the ranges back to back from an odd address inside a buffer of `fill`.
    Everything but the streams themselves must still be `fill`."""
    n, lead = len(blocks), 3
    room = [tabular.snappy_bound(len(b)) for b in blocks] if room is None else room
    src = np.frombuffer(b"\x55" * lead + b"".join(blocks), dtype=np.uint8).copy()
    src_offsets = (lead + np.concatenate([[0], np.cumsum([len(b) for b in blocks])])).astype(np.int64)
    dst_offsets = (5 + np.concatenate([[0], np.cumsum(room)])).astype(np.int64)
    dst = np.full(int(dst_offsets.max()) + 7, fill, dtype=np.uint8)
    sizes, status = np.full(n, 99, dtype=np.int64), np.full(n, 99, dtype=np.int32)
    if form == "host":
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)  # noqa: E731
        _capi.check(_capi.lib().oxh_snappy_compress_host(ctx.handle, n, src.ctypes.data, u64(src_offsets), dst.ctypes.data, u64(dst_offsets),
                                                         u64(sizes), status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "oxh_snappy_compress_host")
    else:
        import torch

        up = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
        d_dst, d_sizes, d_status = up(dst), up(sizes), up(status)
        tabular.snappy_compress_device(up(src), up(src_offsets), d_dst, up(dst_offsets), d_sizes, d_status, ctx=ctx, stream=ctx.stream)
        dst, sizes, status = d_dst.cpu().numpy(), d_sizes.cpu().numpy(), d_status.cpu().numpy()
    streams, untouched = [], np.ones(len(dst), dtype=bool)
    for k in range(n):
        lo = int(dst_offsets[k])
        streams.append(dst[lo:lo + int(sizes[k])].tobytes())
        untouched[lo:lo + int(sizes[k])] = False
    assert np.all(dst[untouched] == fill), "a byte outside the streams was written"
    return streams, [int(s) for s in sizes], [int(s) for s in status]


def check(blocks, result):
    streams, sizes, status = result
    assert status == [0] * len(blocks)
    assert [k for k, (b, s) in enumerate(zip(blocks, streams)) if len(s) > tabular.snappy_bound(len(b)) or S.inflate(s, len(b)) != b] == []


@pytest.mark.parametrize("form", FORMS)
def test_all_cases_in_one_call(ctx, form):
    check(list(CASES.values()), run(ctx, list(CASES.values()), form))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES))
def test_one_block_a_call(ctx, name, form):
    check([CASES[name]], run(ctx, [CASES[name]], form))


@pytest.mark.parametrize("form", FORMS)
def test_sizes_that_follow_from_the_format(ctx, form):
    """A constant block is 64-byte copies at 3 bytes each: at most n / 16 + 16. Random bytes are one literal a fragment:
    at most n + 5 + 3 * ceil(n / 65536). Two equal incompressible fragments share no match -- a copy never crosses the
    cut --: a match inside random bytes has 4 bytes, which saves 1 and costs the literal it splits a second header, so
    the stream has at least the bytes of both fragments."""
    constant = [bytes([200]) * n for n in (4096, 65536, 100000)]
    random = [pat(n, 3) for n in (60, 65536, 65537, 200000)]
    _, sizes, _ = run(ctx, constant + random + [CASES["period_65536"]], form)
    assert [s <= len(b) // 16 + 16 for s, b in zip(sizes, constant)] == [True] * 3 and sizes[1] <= 3077, sizes
    assert [s <= len(b) + 5 + 3 * -(-len(b) // 65536) for s, b in zip(sizes[3:], random)] == [True] * 4, sizes
    assert sizes[-1] >= 2 * 65536, sizes


@pytest.mark.parametrize("form", FORMS)
def test_more_blocks_than_the_grid(ctx, form):
    """3 000 tiny blocks over a grid capped at 2 048 waves: the loops' second round."""
    blocks = [period(1 + k % 9, k % 41) for k in range(3000)]
    check(blocks, run(ctx, blocks, form))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("room", ["one byte below the bound", "decreasing"])
def test_refused_range_between_two_good_ones(ctx, room, form):
    blocks = [CASES["text"], pat(500), CASES["period_7"]]
    bounds = [tabular.snappy_bound(len(b)) for b in blocks]
    rooms = [bounds[0], bounds[1] - 1, bounds[2]] if room != "decreasing" else [bounds[0] + 10, -10, bounds[2]]
    streams, sizes, status = run(ctx, blocks, form, room=rooms)
    assert status == [0, RANGE, 0] and sizes[1] == 0
    assert [S.inflate(streams[k], len(blocks[k])) for k in (0, 2)] == [blocks[0], blocks[2]]


def test_the_same_bytes_every_time_and_in_both_forms(ctx):
    blocks = [CASES[k] for k in ("text", "mixed_131073", "period_2049", "random_257", "run_of_100000", "mixed_5")]
    results = [run(ctx, blocks, form, fill=fill)[:2] for form in FORMS for fill in (0x00, 0xFF, 0xFF)]
    assert all(r == results[0] for r in results)


def test_other_decoders_read_the_streams(ctx):
    blocks = [CASES[k] for k in ("text", "mixed_131073", "period_65536", "run_of_100000", "mixed_0")]
    streams = tabular.snappy_compress(blocks, ctx=ctx)
    assert tabular.snappy_inflate(streams, ctx=ctx) == blocks   # the project's own kernel
    try:   # a second opinion where pyarrow imports
        import pyarrow as pa
    except ImportError:
        return
    codec = pa.Codec("snappy")
    assert [codec.decompress(s, decompressed_size=len(b)).to_pybytes() for s, b in zip(streams, blocks)] == blocks
    assert len(codec.compress(bytes([200]) * 65536)) == 3077   # the reference codec's size for the constant fragment
