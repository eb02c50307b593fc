"""The batched Snappy inflate on the GPU (oxh_snappy_inflate_*, oxen_amd/csrc/snappy_inflate.hip) against a plain
byte-by-byte decoder (tests/_snappy_cases.py): hand-built streams for every element form, length class and edge of the
kernel's 1 KiB window and 64-cell batch; every malformed cause between two good blocks; more blocks than the grid; and
pyarrow's compressor's streams where it imports."""
import numpy as np
import pytest

import _parquet_cases as K
import _snappy_cases as S
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
FORMS = ["host", "device"]


def pat(n, seed=1):   # n bytes no copy of which equals another part by accident
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def mixed(count):   # `count` elements: literals and copies in turn
    return [("lit", pat(3, k)) if k % 2 == 0 else ("copy", 1 + k % 3, 1 + k % 3, 4 + k % 7) for k in range(count)]


CASES = {**{"literal_%d" % n: [("lit", pat(n))] for n in (1, 60, 61, 256, 257, 65536, 65537)},
         "literal_small_in_4_bytes": [("lit", b"abc", 4)],
         "copy_01": [("lit", pat(2047)), ("copy", 1, 1, 4), ("copy", 1, 2047, 11), ("copy", 1, 2047, 4), ("copy", 1, 1, 11)],
         "copy_10": [("lit", pat(65535)), ("copy", 2, 1, 1), ("copy", 2, 65535, 64), ("copy", 2, 1, 64), ("copy", 2, 65535, 1)],
         "copy_11": [("lit", pat(70000)), ("copy", 3, 70000, 64), ("copy", 3, 5, 9)],
         "overlap": [e for o in (1, 2, 3, 7, 64, 63) for e in (("lit", pat(o, o)), ("copy", 2, o, 64))],
         "copy_of_a_literal_of_its_batch": [("lit", b"hello world!"), ("copy", 1, 12, 8)],
         "chain_of_200": [("lit", pat(7))] + [("copy", 2, 7, 7)] * 200,
         **{"window_edge_%d" % n: [("lit", pat(n)), ("copy", 2, n, 10), ("copy", 3, 9, 12), ("lit", b"end")] for n in range(1015, 1027)},
         **{"batch_of_%d" % n: mixed(n) for n in (63, 64, 65, 129)},
         "empty": [], "one_byte": [("lit", b"x")]}
BLOCKS = {name: S.emit(elements) for name, elements in CASES.items()}
GOOD = (S.emit([("lit", b"before"), ("copy", 1, 3, 5)]), S.emit([("lit", pat(300)), ("copy", 2, 300, 40)]))
BAD = {"preamble_of_6_bytes": (b"\x84\x80\x80\x80\x80\x00" + b"\x0cabcd", 4, S.PREAMBLE),
       "preamble_is_not_the_length": (S.emit([("lit", b"abcd")], declared=5), 4, S.PREAMBLE),
       "header_leaves_the_input": (S.emit([("lit", b"abc")], declared=300) + b"\xf4\x01", 300, S.INPUT),
       "literal_leaves_the_input": (S.varint(8) + bytes([7 << 2]) + b"abc", 8, S.INPUT),
       "offset_zero": (S.emit([("lit", b"abcd"), ("copy", 2, 0, 4)]), 8, S.OFFSET_ZERO),
       "offset_beyond": (S.emit([("lit", b"abcd"), ("copy", 2, 5, 4)]), 8, S.OFFSET_BEYOND),
       "element_passes_the_length": (S.emit([("lit", b"abcd"), ("copy", 1, 4, 4)], declared=6), 6, S.OVERRUN),
       "input_ends_early": (S.emit([("lit", b"abcd")], declared=9), 9, S.TRUNCATED)}


@pytest.fixture(scope="module")
def want():   # the reference, computed once and left alone
    return {name: S.inflate(block, sum(len(e[1]) if e[0] == "lit" else e[3] for e in CASES[name])) for name, block in BLOCKS.items()}


@pytest.mark.parametrize("form", FORMS)
def test_all_cases_in_one_call(ctx, want, form):
    names = list(BLOCKS)
    got, status, bad = S.run(ctx, [BLOCKS[k] for k in names], [len(want[k]) for k in names], form)
    assert bad == 0 and status == [0] * len(names)
    assert [k for k, g in zip(names, got) if g != want[k]] == []
    assert tabular.snappy_inflate([BLOCKS[k] for k in names], ctx=ctx) == [want[k] for k in names]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(BLOCKS))
def test_one_block_a_call(ctx, want, name, form):
    assert S.run(ctx, [BLOCKS[name]], [len(want[name])], form) == ([want[name]], [0], 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(BAD))
def test_malformed_block_between_two_good_ones(ctx, name, form):
    block, length, cause = BAD[name]
    with pytest.raises(S.Malformed, match=str(cause)):
        S.inflate(block, length)
    lengths = [11, length, 340]
    got, status, bad = S.run(ctx, [GOOD[0], block, GOOD[1]], lengths, form)
    assert status == [0, cause, 0] and bad == 1 and got[1] == bytes(length)
    assert got[0] == S.inflate(GOOD[0], 11) and got[2] == S.inflate(GOOD[1], 340)
    with pytest.raises(_capi.OxenError, match="block 1"):
        tabular.snappy_inflate([GOOD[0], block, GOOD[1]], ctx=ctx)


@pytest.mark.parametrize("form", FORMS)
def test_more_blocks_than_the_grid(ctx, form):
    """3 000 tiny blocks over a grid capped at 2 048 waves: the block loop's second round."""
    elements = [[("lit", pat(1 + k % 9, k)), ("copy", 1, 1 + k % (1 + k % 9), 4 + k % 8)] for k in range(3000)]
    blocks = [S.emit(e) for e in elements]
    wants = [S.inflate(b, len(e[0][1]) + e[1][3]) for b, e in zip(blocks, elements)]
    got, status, bad = S.run(ctx, blocks, [len(w) for w in wants], form)
    assert bad == 0 and not any(status) and got == wants


@pytest.mark.parametrize("form", FORMS)
def test_streams_of_pyarrow(ctx, form):
    try:   # a second opinion where pyarrow imports
        import pyarrow as pa
    except ImportError:
        return
    codec = pa.Codec("snappy")
    plain = ["".join(K.cells(K.ROWS)["u"]).encode() * 8, bytes(5000), pat(70000)]
    blocks = [codec.compress(p).to_pybytes() for p in plain]
    assert [S.inflate(b, len(p)) for b, p in zip(blocks, plain)] == plain   # the reference reads them as pyarrow does
    assert S.run(ctx, blocks, [len(p) for p in plain], form) == (plain, [0, 0, 0], 0)
