"""The row filter on the GPU (oxh_filter_rows_*, oxen_amd/csrc/filter_rows.hip; oxen_amd.tabular): idx, mask and
the two stats of both forms are compared for EXACT equality with the restatement of tests/_filterrows.py, a plain
Python evaluation row by row -- the complete outputs: idx past `selected` must keep its sentinels and the mask's
bits past nrows must be zero. The edges of the grid and of the scan are read from the sources."""
import functools
import json
import os
import re
import struct

import numpy as np
import pytest

import _filterrows as F
import _grouprows
import _rowhash
import _sortrows
import _take
from _grouprows import strings
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "df_filter.json")
SENTINEL = 0x5A5A5A5A
ALL_OPS = [F.EQ, F.NE, F.LT, F.LE, F.GT, F.GE]
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("filter_rows.hip", "keyed_diff.hip")}
CAP = 2048                                    # the most workgroups of a grid-stride launch and of the scan
SCAN_PER = int(re.search(r"constexpr uint32_t kScanPer = (\d+), kScanTile = 256 \* kScanPer;", SOURCES["keyed_diff.hip"]).group(1))
SCAN_TILE = 256 * SCAN_PER
G = CAP * 256                                 # rows of one round of a grid-stride kernel at one row per lane: the emit
WAVE_BLOCKS = int(re.search(r"constexpr uint32_t kFilterWaveBlocks = (\d+), kFilterGroupRows = 256 \* kFilterWaveBlocks;",
                            SOURCES["filter_rows.hip"]).group(1))
GE = G * WAVE_BLOCKS                          # rows of one round of the evaluate: every wave on WAVE_BLOCKS blocks


# ---------------------------------------------------------------- helpers
def tensor(a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        a = a.view(np.uint8)
    return torch.from_numpy(a.copy()).to("cuda:0")


def device_column(c):
    return Column(c.kind, c.nrows, tensor(c.values), tensor(c.offsets), tensor(c.validity), c.value_bit, c.validity_bit)


class Got:
    def __init__(self, rc, idx, mask, stats):
        self.rc, self.idx, self.mask, self.stats = rc, idx, mask, stats


def raw_call(ctx, form, cols, terms, logical=(), orders=None, want_idx=True, want_mask=True, stream=None):
    """The ABI itself, the outputs filled with sentinels first: the status, the WHOLE idx array (nrows entries),
    the mask as bytes and stats2 (7s where the call wrote none)."""
    import torch

    n = cols[0].nrows
    words = -(-n // 64)
    order_words, term_tables = tabular._filter_tables(cols, terms, logical, orders)
    stats = np.full(2, 7, dtype=np.uint64)
    L = _capi.lib()
    if form == "host":
        keep = []

        def ptr(a):
            if a is None:
                return None
            keep.append(np.ascontiguousarray(a))
            return keep[-1].ctypes.data if keep[-1].size else None

        idx = np.full(n, SENTINEL, dtype=np.uint32)
        mask = np.full(words, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        rc = L.oxh_filter_rows_host(ctx.handle, n, len(cols), *tabular._tables(cols, ptr), order_words, *term_tables,
                                    idx.ctypes.data if want_idx else None, mask.ctypes.data if want_mask else None,
                                    stats.ctypes.data_as(_capi._u64p))
        return Got(rc, idx, mask.view(np.uint8), tuple(stats.tolist()))
    dev = [device_column(c) for c in cols]
    idx = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
    mask = torch.full((words,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    rc = L.oxh_filter_rows_device(ctx.handle, n, len(cols), *tabular._tables(dev, ptr), order_words, *term_tables,
                                  idx.data_ptr() if want_idx else None, mask.data_ptr() if want_mask else None,
                                  stats.ctypes.data_as(_capi._u64p), ctx.stream if stream is None else stream)
    torch.cuda.synchronize()
    return Got(rc, idx.cpu().numpy().view(np.uint32), mask.cpu().numpy().view(np.uint8), tuple(stats.tolist()))


UNTOUCHED_MASK = 0xA5


def same(got, want, who, want_idx=True, want_mask=True, rc=_capi.OXH_OK):
    assert got.rc == rc, (who, got.rc, _capi.lib().oxh_last_error())
    assert got.stats == want.stats, (who, got.stats, want.stats)
    n = got.idx.size
    expect = np.concatenate([want.idx, np.full(n - want.idx.size, SENTINEL, np.uint32)]) if want_idx else np.full(n, SENTINEL, np.uint32)
    if not np.array_equal(got.idx, expect):
        at = int(np.nonzero(got.idx != expect)[0][0])
        raise AssertionError((who, "idx: first difference at", at, got.idx[at:at + 4].tolist(), expect[at:at + 4].tolist()))
    expect = want.mask if want_mask else np.full(want.mask.size, UNTOUCHED_MASK, np.uint8)
    assert got.mask.size == expect.size == 8 * -(-n // 64), who
    if not np.array_equal(got.mask, expect):
        at = int(np.nonzero(got.mask != expect)[0][0])
        raise AssertionError((who, "mask: first difference at byte", at, got.mask[at:at + 4].tolist(), expect[at:at + 4].tolist()))


def check(ctx, cols, terms, logical=(), orders=None, forms=FORMS):
    """Both forms against the restatement; returns the restatement."""
    cols = [c if isinstance(c, Column) else column(c) for c in cols]
    orders = [F.SIGNED] * len(cols) if orders is None else list(orders)
    want = F.filter_rows(cols, terms, logical, orders)
    for form in forms:
        same(raw_call(ctx, form, cols, terms, logical, orders), want, (form, terms, list(logical)))
    return want


def with_nulls(c, rng, bit=5):
    """A third of the rows null, the validity bitmap's row 0 at `bit`."""
    return c._replace(validity=_rowhash.packed_at(rng.random(c.nrows) > 1 / 3, bit), validity_bit=bit)


def f64_word(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def f32_word(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


# ---------------------------------------------------------------- 1. row counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_row_counts(ctx, n):
    """Around a wave's 64-row block and a workgroup's four: the last mask word is partly filled, its tail bits are
    zero, idx past `selected` keeps its sentinels. Int32 with nulls; about half the rows, all rows, no row."""
    rng = np.random.default_rng(n)
    col = with_nulls(column(rng.integers(-50, 50, size=n).astype(np.int32)), rng, bit=3)
    want = check(ctx, [col], [(0, F.GE, 0)])
    assert want.stats[0] + want.stats[1] <= n and want.mask.size == 8 * -(-n // 64)
    tail_bits = np.unpackbits(want.mask, bitorder="little")[n:]
    assert not tail_bits.any()
    plain = column(rng.integers(-50, 50, size=n).astype(np.int32))
    assert check(ctx, [plain], [(0, F.GE, (-50) & 0xFFFFFFFF)]).stats == (n, 0)
    assert check(ctx, [plain], [(0, F.GT, 50)]).stats == (0, 0)
    last = np.zeros(n, dtype=np.int32)
    last[-1] = 1
    assert check(ctx, [column(last)], [(0, F.EQ, 1)]).idx.tolist() == [n - 1]


# ---------------------------------------------------------------- 2. every kind x every operator x three literals
NAN64 = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF5A5A5A5A5A5A5]
NAN32 = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA55AA5]


@functools.lru_cache(maxsize=None)
def kinds_frame():
    """Every OXH_COL_* kind and order class, a third of the rows null in each column, the validity bitmaps and the
    boolean's values starting at bit offsets that are no multiple of 8, offsets[0] != 0, null byte cells with
    bytes underneath. For each column: (Column, order, literals) with literals below all, equal to some, above all
    values (floats: -inf, -0.0, a middle value, +inf, a NaN -- nothing is below -inf or above NaN)."""
    n = 257 + 64
    rng = np.random.default_rng(22)
    i8 = rng.choice(np.array([-100, -1, 1, 5, 100], dtype=np.int8), size=n)       # -1 is 0xFF
    i32 = rng.integers(-1000, 1000, size=n).astype(np.int32)
    i64 = (rng.integers(-1000, 1000, size=n).astype(np.int64) << 33) + 1
    f64 = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, 2.5, np.inf, -np.inf, 5e-324], dtype=np.float64), size=n).view(np.uint64)
    nan_at = rng.random(n) < 0.2
    f64[nan_at] = rng.choice(np.array(NAN64, dtype=np.uint64), size=int(nan_at.sum()))
    f32 = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, 2.5, np.inf, -np.inf, 1e-45], dtype=np.float32), size=n).view(np.uint32)
    f32[nan_at] = rng.choice(np.array(NAN32, dtype=np.uint32), size=int(nan_at.sum()))
    words = [b"", b"a", b"ab", b"abc", b"a\0", b"\xff\xfe", b"longer than eight bytes", b"longer than eight bytez"]
    s32 = strings([words[k] for k in rng.integers(0, len(words), size=n)], F.BYTES32, rng.random(n) > 1 / 3, 5, lead=b"LEAD!")
    s64 = strings([words[k] for k in rng.integers(0, len(words), size=n)], F.BYTES64, rng.random(n) > 1 / 3, 2, lead=b"xy")
    flag = with_nulls(Column(F.BOOL, n, _rowhash.packed_at(rng.random(n) < 0.5, 13), None, None, 13, 0), rng, bit=7)
    assert s32.offsets[0] == 5 and s64.offsets[0] == 2 and flag.value_bit == 13 and flag.validity_bit == 7
    assert (i8 == -1).any() and nan_at.sum() > 8 and (f64 == f64_word(-0.0)).any() and (f64 == 0).any()
    return {
        "i8 signed": (with_nulls(column(i8), rng, bit=1), F.SIGNED, [0x80, 0xFF, 127]),            # -128, -1, 127
        "i8 unsigned": (with_nulls(column(i8), rng, bit=2), F.UNSIGNED, [0, 0xFF, 0x7F]),          # 0, 255 (the most), 127 (a middle)
        "i32": (with_nulls(column(i32), rng, bit=3), F.SIGNED, [(-1001) & 0xFFFFFFFF, int(i32[7]) & 0xFFFFFFFF, 1000]),
        "i64": (with_nulls(column(i64), rng, bit=4), F.SIGNED, [(-(1 << 62)) & (2**64 - 1), int(i64[9]) & (2**64 - 1), 1 << 62]),
        "i64 unsigned": (with_nulls(column(i64), rng, bit=6), F.UNSIGNED, [0, int(i64[9]) & (2**64 - 1), 2**64 - 1]),
        "f32": (with_nulls(Column(4, n, f32.view(np.float32)), rng, bit=5), F.FLOAT,
                [f32_word(-np.inf), f32_word(-0.0), f32_word(1.5), f32_word(2.0), f32_word(np.inf), 0xFFC12345]),
        "f64": (with_nulls(Column(8, n, f64.view(np.float64)), rng, bit=7), F.FLOAT,
                [f64_word(-np.inf), f64_word(-0.0), f64_word(1.5), f64_word(2.0), f64_word(np.inf), 0x7FF8000000000123]),
        "f64 as bits": (Column(8, n, f64.view(np.float64)), F.UNSIGNED, [f64_word(-0.0), f64_word(0.0), NAN64[1]]),
        "bool": (flag, F.SIGNED, [0, 1]),
        "bytes32": (s32, F.SIGNED, [b"", b"ab", b"a\0", b"longer than eight bytes", b"longer than eight bytf", b"\xff\xff"]),
        "bytes64": (s64, F.SIGNED, [b"", b"a", b"abcd", b"longer than eight bytez", b"\xff\xfe\x00"]),
    }


@pytest.mark.parametrize("name", ["i8 signed", "i8 unsigned", "i32", "i64", "i64 unsigned", "f32", "f64", "f64 as bits", "bool",
                                  "bytes32", "bytes64"])
def test_every_kind_operator_and_literal(ctx, name):
    col, order, literals = kinds_frame()[name]
    seen = set()
    for lit in literals:
        for op in ALL_OPS:
            want = check(ctx, [col], [(0, op, lit)], orders=[order])
            seen.add(want.stats[0])
            assert want.stats[1] == (col.nrows - int(F.bits(col.validity, col.validity_bit, col.nrows).sum()) if col.validity is not None else 0)
    assert len(seen) > 3 and 0 in seen      # the literals do select differently, and some operator selects nothing
    values = F.cells(col, order)
    present = [v for v in values if v is not None]
    if name == "i8 signed":
        assert check(ctx, [col], [(0, F.LT, 0)], orders=[order]).stats[0] == sum(1 for v in present if v < 0) > 0
    if name == "i8 unsigned":      # 0xFF is the largest there: nothing is above it
        assert check(ctx, [col], [(0, F.GT, 0xFF)], orders=[order]).stats[0] == 0 and max(present) == 255
    if name in ("f32", "f64"):
        nan = literals[-1]
        assert check(ctx, [col], [(0, F.EQ, nan)], orders=[order]).stats[0] == sum(1 for v in present if v == (1, 0.0)) > 8
        assert check(ctx, [col], [(0, F.GT, literals[4])], orders=[order]).stats[0] == sum(1 for v in present if v == (1, 0.0))
        assert check(ctx, [col], [(0, F.EQ, literals[1])], orders=[order]).stats[0] == sum(1 for v in present if v == (0, 0.0)) > 8
    if name == "f64 as bits":
        assert check(ctx, [col], [(0, F.EQ, literals[0])], orders=[order]).stats[0] < sum(1 for v in F.cells(col, F.FLOAT) if v == (0, 0.0))


# ---------------------------------------------------------------- 3. string cells
@pytest.mark.parametrize("kind", [F.BYTES32, F.BYTES64])
def test_string_cells(ctx, kind):
    """"", a proper prefix of the literal, an embedded NUL, a 300-byte cell, cells that share 8 and 16 bytes with
    the literal and differ right behind them or only in length, and the literal "" -- every operator."""
    lit = b"0123456789abcdefXYZ"            # 19 bytes: two 8-byte steps and a tail of 3
    big = lit + b"-" * (300 - len(lit))
    cells = [b"", lit, lit[:5], lit[:8], lit[:16], lit[:18], lit + b"\0", lit[:8] + b"\0", lit[:7] + b"\xff", b"01234567" + b"9",
             lit[:16] + b"XY[", lit[:16] + b"XYY", lit[:16] + b"\0YZ", lit[:8] + b"8" + lit[9:], b"\0", b"\0\0", big, big[:-1] + b".",
             b"1", b"/", lit[:15] + b"g", lit[:15] + b"e" + lit[16:]] * 3
    valid = [True] * len(cells)
    valid[3] = valid[30] = False
    col = strings(cells, kind, valid, 3, lead=b"abc")
    for literal in (lit, b"", big, lit[:8], lit[:16], lit[:16] + b"X", b"\0", lit + b"\0"):
        for op in ALL_OPS:
            want = check(ctx, [col], [(0, op, literal)])
            assert want.stats[1] == 2
    assert check(ctx, [col], [(0, F.EQ, b"")]).stats[0] == 3 and check(ctx, [col], [(0, F.GE, b"")]).stats[0] == len(cells) - 2
    assert check(ctx, [col], [(0, F.EQ, big)]).stats[0] == 3 and check(ctx, [col], [(0, F.LT, lit)]).stats[0] > 20


# ---------------------------------------------------------------- 4. logic
def test_kleene_on_null_cells(ctx):
    """null && false is false (dropped, and not counted as null), null || true is true (kept), null || false and
    null && true are null (dropped, counted) -- and != on a null cell is null, not true."""
    n = 130
    a = column(np.arange(n, dtype=np.int64), validity=[i % 3 != 0 for i in range(n)])
    b = column(np.array([i % 2 == 0 for i in range(n)]))
    nulls = sum(1 for i in range(n) if i % 3 == 0)
    ge0 = (0, F.GE, 0)                                   # true on every present cell, null on the others
    want = check(ctx, [a, b], [ge0, (1, F.EQ, 0)], [F.AND])          # null && (b == false)
    assert want.stats == (sum(1 for i in range(n) if i % 3 and i % 2), sum(1 for i in range(n) if i % 3 == 0 and i % 2))
    want = check(ctx, [a, b], [ge0, (1, F.EQ, 1)], [F.OR])           # null || (b == true): kept where b is true
    assert want.stats == (sum(1 for i in range(n) if i % 3 or i % 2 == 0), sum(1 for i in range(n) if i % 3 == 0 and i % 2))
    want = check(ctx, [a, b], [(0, F.LT, 0), (1, F.EQ, 1)], [F.OR])  # false-or-null || b
    assert want.stats == (n // 2, sum(1 for i in range(n) if i % 3 == 0 and i % 2))
    assert check(ctx, [a], [(0, F.NE, 5)]).stats == (n - nulls - 1, nulls)
    assert check(ctx, [a, a], [(0, F.NE, 5), (1, F.EQ, 5)], [F.OR]).stats == (n - nulls, nulls)


def test_the_fold_has_no_precedence(ctx):
    """a || b && c is (a || b) && c: with a true and c false the row is dropped, where && before || would keep it."""
    n = 200
    rng = np.random.default_rng(4)
    cols = [with_nulls(column(rng.integers(0, 2, size=n).astype(np.int8)), rng, bit=k + 1) for k in range(3)]
    one = lambda c: (c, F.EQ, 1)  # noqa: E731
    want = check(ctx, cols, [one(0), one(1), one(2)], [F.OR, F.AND])
    with_precedence = [F.or3(a, F.and3(b, c)) for a, b, c in zip(*[[None if v is None else v == 1 for v in F.cells(c)] for c in cols])]
    assert [r is True for r in want.results] != [r is True for r in with_precedence]
    check(ctx, cols, [one(0), one(1), one(2)], [F.AND, F.OR])
    check(ctx, cols, [one(2), one(0), one(1), one(2), one(0)], [F.OR, F.AND, F.OR, F.AND])


def test_sixteen_terms_and_seventeen(ctx):
    """The most terms a call takes, over every kind at once with 16 byte literals, && and || alternating; one more
    is OXH_ERR_INVALID with nothing written."""
    frame = kinds_frame()
    names = ["i8 signed", "bytes32", "f64", "bool", "bytes64", "i32", "i64", "f32"]
    cols = [frame[x][0] for x in names]
    orders = [frame[x][1] for x in names]
    terms = [(k % 8, ALL_OPS[(k * 5 + 3) % 6], frame[names[k % 8]][2][1 if k < 8 else -1]) for k in range(16)]
    logical = [k & 1 ^ 1 for k in range(15)]
    want = check(ctx, cols, terms, logical, orders)
    assert 0 < want.stats[0] < cols[0].nrows and want.stats[1] > 0
    # 16 byte terms that fill OXH_FILTER_MAX_LITERAL_BYTES to the byte, each literal at an odd place
    text = strings([bytes([65 + k % 7]) * (250 + k % 9) for k in range(300)])
    lits = [bytes([65 + t % 7]) * (255 if t < 15 else 4096 - 15 * 255) for t in range(16)]
    assert sum(len(b) for b in lits) == _capi.OXH_FILTER_MAX_LITERAL_BYTES
    want = check(ctx, [text], [(0, [F.EQ, F.GT, F.LE][t % 3], lits[t]) for t in range(16)], [F.OR] * 15)
    assert 0 < want.stats[0] <= 300
    for form in FORMS:
        got = raw_call(ctx, form, cols, terms + [terms[0]], logical + [F.AND], orders)
        assert got.rc == _capi.OXH_ERR_INVALID and b"OXH_FILTER_MAX_TERMS" in _capi.lib().oxh_last_error()
        assert got.stats == (7, 7) and (got.idx == SENTINEL).all() and (got.mask == UNTOUCHED_MASK).all()


# ---------------------------------------------------------------- 5. selections and outputs
@pytest.mark.parametrize("n", [64 * 5, 64 * 5 + 37])
def test_selections_none_all_alternating_last(ctx, n):
    values = np.arange(n, dtype=np.int64)
    col = column(values)
    assert check(ctx, [col], [(0, F.LT, 0)]).stats == (0, 0)
    assert check(ctx, [col], [(0, F.GE, 0)]).idx.tolist() == list(range(n))
    alt = check(ctx, [column((values & 1).astype(np.int8))], [(0, F.EQ, 1)])
    assert alt.idx.tolist() == list(range(1, n, 2)) and set(alt.mask[:n // 8].tolist()) == {0xAA}
    assert check(ctx, [col], [(0, F.EQ, n - 1)]).idx.tolist() == [n - 1]
    assert check(ctx, [col], [(0, F.EQ, 0)]).idx.tolist() == [0]


def test_each_output_null_in_turn(ctx):
    """idx alone, the mask alone, neither (the stats alone): what is not asked for is not written, what is asked
    for is the restatement's."""
    n = 64 * 7 + 11
    rng = np.random.default_rng(5)
    cols = [with_nulls(column(rng.integers(0, 90, size=n).astype(np.int64)), rng), strings([b"ab"[:k] for k in rng.integers(0, 3, size=n)])]
    terms, logical = [(0, F.LT, 40), (1, F.NE, b"a")], [F.AND]
    want = F.filter_rows(cols, terms, logical)
    assert 0 < want.stats[0] < n and want.stats[1] > 0
    for form in FORMS:
        for want_idx, want_mask in ((True, True), (True, False), (False, True), (False, False)):
            got = raw_call(ctx, form, cols, terms, logical, want_idx=want_idx, want_mask=want_mask)
            same(got, want, (form, want_idx, want_mask), want_idx, want_mask)


def test_the_python_layer_and_a_stream_of_the_caller(ctx):
    """`filter_rows` and `filter_rows_device`: idx a view of length `selected`, the mask as uint8; the device form on
    a stream that is neither the default one nor the context's."""
    import torch

    n = 1000
    rng = np.random.default_rng(6)
    cols = [with_nulls(column(rng.standard_normal(n)), rng), column(rng.random(n) < 0.5)]
    terms, logical = [(0, F.GT, f64_word(0.25)), (1, F.EQ, 1)], [F.OR]
    want = F.filter_rows(cols, terms, logical, [F.FLOAT, F.SIGNED])
    host = tabular.filter_rows(cols, terms, logical, want_mask=True, ctx=ctx)      # the orders: from the dtypes
    assert host.idx.dtype == np.uint32 and host.mask.dtype == np.uint8 and tuple(host.stats) == want.stats
    assert np.array_equal(host.idx, want.idx) and np.array_equal(host.mask, want.mask)
    assert tabular.filter_rows(cols, terms, logical, ctx=ctx).mask is None
    only_mask = tabular.filter_rows(cols, terms, logical, want_mask=True, want_idx=False, ctx=ctx)
    assert only_mask.idx is None and np.array_equal(only_mask.mask, want.mask)
    dev = [device_column(c)._replace(values=tensor(c.values).view(torch.float64) if c.kind == 8 else tensor(c.values)) for c in cols]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream not in (0, ctx.stream)
    torch.cuda.synchronize()
    got = tabular.filter_rows_device(dev, terms, logical, want_mask=True, stream=stream, ctx=ctx)
    assert got.idx.is_cuda and got.idx.dtype == torch.int32 and got.idx.numel() == want.stats[0] and got.mask.dtype == torch.uint8
    assert np.array_equal(got.idx.cpu().numpy().view(np.uint32), want.idx) and np.array_equal(got.mask.cpu().numpy(), want.mask)
    assert tuple(got.stats) == want.stats
    same(raw_call(ctx, "device", cols, terms, logical, [F.FLOAT, F.SIGNED], stream=stream.cuda_stream), want, "raw, own stream")
    # idx feeds the device take as it is; the mask is a boolean column's values
    taken = tabular.take_device([dev[0]], got.idx, stream=ctx.stream, ctx=ctx)[0]
    present = F.bits(cols[0].validity, cols[0].validity_bit, n)[want.idx]     # a null cell's value is not compared
    assert np.array_equal(taken.values.cpu().numpy().view(np.float64)[present], cols[0].values[want.idx][present]) and not present.all()
    flagged = tabular.filter_rows([Column(F.BOOL, n, host.mask)], [(0, F.EQ, 1)], ctx=ctx)
    assert np.array_equal(flagged.idx, want.idx)


# ---------------------------------------------------------------- 6. bad offsets
def test_decreasing_offsets(ctx):
    """The host form refuses and writes nothing; the device form treats the pair as an empty cell (b"", not a
    null), finishes and returns OXH_ERR_INVALID with the outputs of that frame; the next call is fine."""
    good = column(["ab", "cd", "", "g", "", "ab"])
    broken = good._replace(offsets=np.array([0, 2, 4, 3, 5, 5, 7], dtype=np.int32))   # a decreasing pair at row 2
    other = column(np.array([1, 1, 2, 1, 2, 1], dtype=np.int8))
    terms, logical = [(1, F.LE, b"ab"), (0, F.EQ, 2)], [F.AND]
    want = F.filter_rows([other, broken], terms, logical, empty={1: {2}})
    assert want.idx.tolist() == [2, 4] and want.stats == (2, 0)
    got = raw_call(ctx, "device", [other, broken], terms, logical)
    assert b"offsets" in _capi.lib().oxh_last_error()
    same(got, want, "device", rc=_capi.OXH_ERR_INVALID)
    got = raw_call(ctx, "host", [other, broken], terms, logical)
    assert got.rc == _capi.OXH_ERR_INVALID and b"decrease" in _capi.lib().oxh_last_error()
    assert got.stats == (7, 7) and (got.idx == SENTINEL).all() and (got.mask == UNTOUCHED_MASK).all()
    with pytest.raises(_capi.OxenError, match="decrease"):
        tabular.filter_rows([other, broken], terms, logical, ctx=ctx)
    # a broken column that no term names is never read
    check(ctx, [other, broken], [(0, F.EQ, 2)], forms=["device"])
    check(ctx, [other, good], terms, logical)


# ---------------------------------------------------------------- 7. golden frames and the composition
def golden_frame(case, which="frame"):
    out = {}
    for name, values in case[which].items():
        dt = case["dtypes"][name]
        out[name] = column(values) if dt == "str" else column(np.array(values, dtype={"f64": np.float64, "bool": bool}[dt]))
    return out


def test_filter_df_reproduces_the_reference_s_frames(ctx):
    """The three expected frames of tabular.rs:1709-1800, through `filter_df`."""
    fx = json.load(open(GOLDEN))
    assert len(fx["cases"]) == 3
    for case in fx["cases"]:
        got = tabular.filter_df(golden_frame(case), case["query"], ctx=ctx)
        want = golden_frame(case, "expected")
        assert list(got) == list(want), case["name"]
        for name, c in want.items():
            assert got[name].kind == c.kind and _take.pylist(got[name]) == _take.pylist(c), (case["name"], name)
    none = tabular.filter_df(golden_frame(fx["cases"][2]), "label == cat", ctx=ctx)
    assert all(c.nrows == 0 for c in none.values())


def test_filter_then_unique_then_sort(ctx):
    """`oxen df --filter "label != unknown && min_x > 0.5 || is_correct == true" --unique image --sort image`:
    `filter_df` -> `unique` -> `sort_by` against the three restatements composed."""
    n = 3000
    rng = np.random.default_rng(7)
    labels = ["dog", "cat", "unknown", "", "person"]
    frame = {
        "image": column(["%04d.jpg" % k for k in rng.integers(0, 400, size=n)]),
        "label": strings([labels[k].encode() for k in rng.integers(0, 5, size=n)], valid=rng.random(n) > 0.1, bit=3),
        "min_x": with_nulls(column(np.round(rng.random(n), 2)), rng, bit=6),
        "is_correct": column(rng.random(n) < 0.3),
    }
    query = "label != unknown && min_x > 0.5 || is_correct == true"
    got = tabular.sort_by(tabular.unique(tabular.filter_df(frame, query, ctx=ctx), "image", ctx=ctx), "image", ctx=ctx)
    cols = list(frame.values())
    terms, logical = tabular.filter_terms(frame, query)
    assert terms == [(1, F.NE, b"unknown"), (2, F.GT, f64_word(0.5)), (3, F.EQ, 1)] and logical == [F.AND, F.OR]
    sel = F.filter_rows(cols, terms, logical, [F.SIGNED, F.SIGNED, F.FLOAT, F.SIGNED])
    assert 0 < sel.stats[0] < n and sel.stats[1] > 0
    plain = lambda taken: [Column(t.kind, t.nrows, t.values, t.offsets, t.validity) for t in taken]  # noqa: E731
    kept = plain(_take.take(cols, sel.idx))
    firsts = plain(_take.take(kept, _grouprows.group_rows([kept[0]]).first_idx))
    perm, _ = _sortrows.sort_indices([firsts[0]])
    want = plain(_take.take(firsts, perm))
    assert list(got) == list(frame) and got["image"].nrows == want[0].nrows > 100
    for name, w in zip(frame, want):
        assert _take.pylist(got[name], text=False) == _take.pylist(w, text=False), name


# ---------------------------------------------------------------- 8. edges read from the sources
def test_the_caps_the_edges_come_from():
    """A changed cap, block or tile fails here, loudly, instead of moving an edge away from the cases below."""
    src = SOURCES["filter_rows.hip"]
    (cap,) = re.findall(r"unsigned stride_grid\(uint64_t n\) \{ return \(unsigned\)std::min<uint64_t>\(\(n \+ 255\) / 256, (\d+)\); \}", src)
    assert int(cap) == CAP
    (cap,) = re.findall(r"unsigned eval_grid\(uint64_t n\) \{ return \(unsigned\)std::min<uint64_t>\(\(n \+ oxh::kFilterGroupRows - 1\) / oxh::kFilterGroupRows, (\d+)\); \}", src)
    assert int(cap) == CAP and WAVE_BLOCKS == 4
    assert src.count("<<<stride_grid(n), 256, 0, st>>>") == 1 and src.count("<<<eval_grid(n), 256, 0, st>>>") == 1
    assert src.count("__launch_bounds__(256)") == 2
    assert "exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st)" in src and "mask[i >> 6]" in src
    scan = SOURCES["keyed_diff.hip"]
    scan = scan[scan.index("int exclusive_scan_u32("):]
    (cap,) = re.findall(r"const unsigned grid = \(unsigned\)std::min<uint64_t>\(std::max<uint64_t>\(ntiles, 1\), (\d+)\);", scan[:scan.index("\n}\n")])
    assert int(cap) == CAP and "scan_sums_kernel<<<1, 256, 0, st>>>" in scan
    assert (G, GE, SCAN_TILE) == (524288, 2097152, 2048)
    # the array restatement of the cases below is the plain one
    rng = np.random.default_rng(8)
    values = rng.integers(-128, 128, size=777).astype(np.int8)
    for op in ALL_OPS:
        a, b = array_selection(values, op, -3), F.filter_rows([column(values)], [(0, op, 0xFD)])
        assert np.array_equal(a.idx, b.idx) and np.array_equal(a.mask, b.mask) and a.stats == b.stats


def array_selection(values, op, lit):
    """The restatement for one term on a signed fixed-width column without nulls, by arrays."""
    picked = F.OPS[op](values, lit)
    mask = np.zeros(8 * -(-values.size // 64), dtype=np.uint8)
    packed = np.packbits(picked, bitorder="little")
    mask[:packed.size] = packed
    return F.Selection(np.nonzero(picked)[0].astype(np.uint32), mask, (int(picked.sum()), 0), None)


def check_arrays(ctx, values, op, lit, forms):
    want = array_selection(values, op, lit)
    width = values.dtype.itemsize
    for form in forms:
        same(raw_call(ctx, form, [column(values)], [(0, op, lit & ((1 << (8 * width)) - 1))]), want, (form, values.size, op))
    return want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("edge", [G, GE], ids=["emit", "evaluate"])
def test_rows_past_the_grid(ctx, form, edge):
    """n = G + 65 and n = GE + 65: the 65 rows of the second grid-stride iteration of the emit (one row per lane) and
    of the evaluate (four blocks per wave) -- a whole block and a one-row block -- with their own mask words, counts
    and places; the two sums of both iterations add."""
    n = edge + 65
    rng = np.random.default_rng(9)
    values = rng.integers(-1000, 1000, size=n).astype(np.int32)
    want = check_arrays(ctx, values, F.GT, 300, [form])
    assert (want.idx >= edge).sum() > 10 and want.idx[-1] >= edge
    values[:] = 0
    values[edge:] = 1
    assert check_arrays(ctx, values, F.EQ, 1, [form]).idx.tolist() == list(range(edge, n))


@pytest.mark.parametrize("n", [64 * SCAN_TILE - 64, 64 * SCAN_TILE, 64 * SCAN_TILE + 64])
def test_block_counts_around_one_scan_tile(ctx, n):
    """The per-block counts fill one tile of the scan less a block, exactly, and one block more: the last block's
    base stands on the second tile's sum."""
    assert -(-(n // 64) // SCAN_TILE) == (2 if n > 64 * SCAN_TILE else 1)
    rng = np.random.default_rng(n)
    values = rng.integers(-100, 100, size=n).astype(np.int64)
    want = check_arrays(ctx, values, F.LE, -50, ["device"])
    assert want.idx[-1] >= n - 64 or (values[-64:] > -50).all()
    check_arrays(ctx, values, F.GE, -100, ["device"])      # every row: 64 per block


def test_the_scan_carries_over_the_block_counts(ctx):
    """n = 64 * G + 65 rows of one Int8 column (about 34 MB): G + 2 block counts, so the scan of the counts runs
    over 257 tiles and its sums are scanned with a carry; the evaluate and the emit loop 64 times. About a quarter
    of the rows selected, against the array restatement."""
    n = 64 * G + 65
    assert -(-n // 64) == G + 2 and -(-(G + 2) // SCAN_TILE) == 257
    rng = np.random.default_rng(10)
    values = rng.integers(-128, 128, size=n, dtype=np.int8)
    want = check_arrays(ctx, values, F.LT, -64, ["device"])
    assert n // 5 < want.stats[0] < n // 3 and want.idx[-1] > 64 * G - 64
