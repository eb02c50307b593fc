"""The concat on the GPU (oxh_concat_columns_*, oxen_amd/csrc/concat_columns.hip; oxen_amd.tabular): every output
buffer of both forms is pre-filled with sentinels, with a guard in front and behind, and the WHOLE buffers are
compared for exact equality with the restatement of tests/_concat.py -- a byte written past a defined size shows.
The piece sizes and the grid cap are read from the sources."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import _concat
import _filterrows as F
import _grouprows
import _rowhash
import _take
from _grouprows import strings
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
INVALID, OK = _capi.OXH_ERR_INVALID, _capi.OXH_OK
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("concat_columns.hip", "concat_columns_host.hpp")}
PIECE = int(re.search(r"constexpr uint32_t kConcatPiece = (\d+);", SOURCES["concat_columns_host.hpp"]).group(1))
OFFSET_PIECE = int(re.search(r"constexpr uint32_t kConcatOffsetPiece = (\d+);", SOURCES["concat_columns_host.hpp"]).group(1))
CAP = int(re.search(r"constexpr unsigned kConcatMaxGroups = (\d+);", SOURCES["concat_columns.hip"]).group(1))
GUARD = 64          # sentinel bytes in front of and behind every output buffer (keeps the 8-byte alignment)
SENTINEL = 0xA5
CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_test", "csvs", "mixed_data_types.csv")


# ---------------------------------------------------------------- helpers
def tensor(a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        a = a.view(np.uint8)
    return torch.from_numpy(a.copy()).to("cuda:0")


def device_column(c, cache=None):
    """The column on the device; `cache` keeps one tensor per numpy array, so parts that alias on the host alias
    on the device."""
    def up(a):
        if a is None or cache is None:
            return tensor(a)
        if id(a) not in cache:
            cache[id(a)] = (tensor(a), a)
        return cache[id(a)][0]

    return Column(c.kind, c.nrows, up(c.values), up(c.offsets), up(c.validity), c.value_bit, c.validity_bit)


def sizes_of(want):
    """Per output column the bytes of (values, offsets, validity), from the restatement."""
    return [(t.values.size, 0 if t.offsets is None else t.offsets.size * t.offsets.dtype.itemsize, t.validity.size) for t in want]


class Got:
    def __init__(self, rc, outs, value_bytes, written, err):
        self.rc, self.outs, self.value_bytes, self.written, self.err = rc, outs, value_bytes, written, err


def raw_call(ctx, form, parts, ranges, sizes, capacity=None, outputs=True, stream=None):
    """The ABI itself. sizes: per column the bytes of (values, offsets, validity) the outputs get, each between two
    guards, all of it sentinels; capacity: value_capacity (default: the values' sizes). Returns the status, the
    whole buffers (guards included) as uint8 arrays, value_bytes (7s where the call wrote none) and written."""
    import torch

    kinds = [int(c.kind) for c in parts[0]]
    rows = [p[0].nrows for p in parts]
    first = None if ranges is None else [f for f, _ in ranges]
    count = None if ranges is None else [n for _, n in ranges]
    value_bytes = (ctypes.c_uint64 * len(kinds))(*[7] * len(kinds))
    written = ctypes.c_uint32(7)
    cap = (ctypes.c_uint64 * len(kinds))(*(capacity if capacity is not None else [s[0] for s in sizes]))
    L = _capi.lib()
    if form == "host":
        keep = []

        def ptr(a):
            if a is None:
                return None
            keep.append(np.ascontiguousarray(a))
            return keep[-1].ctypes.data if keep[-1].size else None

        bufs = [[np.full(size + 2 * GUARD, SENTINEL, dtype=np.uint8) for size in s] for s in sizes]
        arrays = [tabular._pointers([b[k].ctypes.data + GUARD for b in bufs]) for k in (0, 1, 2)] if outputs else [None] * 3
        head = tabular._concat_head(parts, kinds, rows, first, count, ptr)
        rc = L.oxh_concat_columns_host(ctx.handle, *head, cap if outputs else None, *arrays, value_bytes, ctypes.byref(written))
        outs = bufs
    else:
        cache = {}
        dev = [[device_column(c, cache) for c in p] for p in parts]
        bufs = [[torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0") for size in s] for s in sizes]
        torch.cuda.synchronize()
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
        arrays = [tabular._pointers([b[k].data_ptr() + GUARD for b in bufs]) for k in (0, 1, 2)] if outputs else [None] * 3
        head = tabular._concat_head(dev, kinds, rows, first, count, ptr)
        rc = L.oxh_concat_columns_device(ctx.handle, *head, cap if outputs else None, *arrays, value_bytes, ctypes.byref(written),
                                         ctx.stream if stream is None else stream)
        torch.cuda.synchronize()
        outs = [[b.cpu().numpy() for b in three] for three in bufs]
    return Got(rc, outs, list(value_bytes), written.value, _capi.lib().oxh_last_error())


def guarded(content):
    g = np.full(GUARD, SENTINEL, dtype=np.uint8)
    return np.concatenate([g, np.ascontiguousarray(content).view(np.uint8).reshape(-1), g])


def assert_same(got, want, who, rc=OK):
    assert got.rc == rc, (who, got.rc, got.err)
    assert got.written == 1 and got.value_bytes == [t.values.size for t in want], (who, got.written, got.value_bytes)
    for c, (t, (values, offsets, validity)) in enumerate(zip(want, got.outs)):
        for name, have, expect in (("values", values, t.values), ("offsets", offsets, t.offsets if t.offsets is not None else np.zeros(0, np.uint8)),
                                   ("validity", validity, t.validity)):
            expect = guarded(expect)
            assert have.size == expect.size, (who, c, name, have.size, expect.size)
            if not np.array_equal(have, expect):
                at = int(np.nonzero(have != expect)[0][0])
                raise AssertionError((who, "column", c, name, "first difference at byte", at - GUARD, "of", expect.size - 2 * GUARD,
                                      have[at:at + 8].tolist(), expect[at:at + 8].tolist()))


def assert_untouched(got, who):
    for three in got.outs:
        for b in three:
            assert (b == SENTINEL).all(), who


def check(ctx, parts, ranges=None, forms=FORMS):
    """Both forms against the restatement; returns the restatement."""
    want = _concat.concat(parts, ranges)
    for form in forms:
        assert_same(raw_call(ctx, form, parts, ranges, sizes_of(want)), want, form)
    return want


def frame(rng, n, kinds, bit=0, nulls=True, cell=7):
    """One part: a column per kind with random cells, a third of the rows null (the values stay underneath), the
    bitmaps' row 0 at `bit` / `bit` + 3, a byte column's offsets not starting at 0."""
    cols = []
    for k, kind in enumerate(kinds):
        valid = rng.random(n) > 1 / 3 if nulls else None
        vbit = bit + k if nulls else 0
        validity = _rowhash.packed_at(valid, vbit, rng) if nulls else None
        if kind in (1, 4, 8):
            cols.append(Column(kind, n, rng.integers(0, 256, n * kind, dtype=np.uint8), None, validity, 0, vbit))
        elif kind == 16:
            cols.append(Column(16, n, _rowhash.packed_at(rng.random(n) > 0.5, bit + 3, rng), None, validity, bit + 3, vbit))
        else:
            cells = [bytes(rng.integers(97, 123, int(l), dtype=np.uint8)) for l in rng.integers(0, cell + 1, n)]
            cols.append(strings(cells, kind, valid, vbit, lead=b"?" * (k + 1)))
    return cols


# ---------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("bit", [0, 1, 7, 8, 63, 64, 65])
def test_bit_packed_outputs_at_every_source_bit_offset(ctx, bit):
    """Part counts 1, 7, 63, 64, 65, 129 and 0 -- an empty part in the middle --, a part without validity between
    two with validity; the boolean's values at bit + 3, each validity bitmap at its own offset."""
    rng = np.random.default_rng(100 + bit)
    counts = [1, 7, 63, 0, 64, 65, 129, 0, 7]
    parts = [frame(rng, n + 5, [16, 1], bit) for n in counts]
    parts[4] = [c._replace(validity=None, validity_bit=0) for c in parts[4]]
    check(ctx, parts, [(3, n) for n in counts])
    check(ctx, [[c._replace(validity=None, validity_bit=0) for c in p] for p in parts], [(3, n) for n in counts])   # no part has validity


def test_one_output_word_drawn_from_64_parts(ctx):
    rng = np.random.default_rng(7)
    parts = [frame(rng, 3, [16], p % 11) for p in range(200)]
    for p in (5, 70, 71):
        parts[p] = [c._replace(validity=None, validity_bit=0) for c in parts[p]]
    check(ctx, parts, [(p % 3, 1) for p in range(200)])


@pytest.mark.parametrize("n", [1, 8, 63, 64, 65])
def test_pad_bits_and_the_byte_wise_last_word(ctx, n):
    rng = np.random.default_rng(n)
    one = frame(rng, n + 2, [16, 4], 5)
    check(ctx, [one], [(1, n)])
    if n > 1:
        check(ctx, [one, one], [(0, n - 1), (n, 1)])           # the same frame as parts 0 and 1
    check(ctx, [frame(rng, n, [16, 8], 0, nulls=False)])           # whole parts, no validity anywhere: all ones, pad bits 0


# ---------------------------------------------------------------- 2. bytes
@pytest.mark.parametrize("kind", [32, 64])
def test_byte_spans_at_every_source_and_destination_alignment(ctx, kind):
    """Source start alignment 0..15 x destination alignment 0..15 x span lengths 0, 1, 15, 16, 17, 255: every part
    is one row of ONE column (the parts alias). Rows 0..15 are fillers of 0..15 bytes; then, per source alignment
    and length, a pad row and the test row. A filler part in front of each test part sets the destination
    alignment, which is the byte total of the parts before. A third of the cells are null and keep their spans."""
    rng = np.random.default_rng(kind)
    lengths = [0, 1, 15, 16, 17, 255]
    cells, at, total = [], {}, 3                                                   # 3 lead bytes: offsets[0] != 0
    for fill in range(16):
        cells.append(bytes(rng.integers(65, 91, fill, dtype=np.uint8)))
        total += fill
    for sa in range(16):
        for length in lengths:
            cells.append(b"-" * ((sa - total) % 16))
            total += len(cells[-1])
            assert total % 16 == sa
            at[sa, length] = len(cells)
            cells.append(bytes(rng.integers(97, 123, length, dtype=np.uint8)))
            total += length
    col = strings(cells, kind, rng.random(len(cells)) > 1 / 3, 3, lead=b"???")
    ranges, out = [], 0
    for sa in range(16):
        for length in lengths:
            for da in range(16):
                fill = (da - out) % 16
                ranges += [(fill, 1), (at[sa, length], 1)]
                out += fill + length
    parts = [[col]] * len(ranges)
    want = check(ctx, parts, ranges)
    assert want[0].values.size == out and len(ranges) == 2 * 16 * 16 * len(lengths)


@pytest.mark.parametrize("kind", [32, 64])
def test_spans_of_one_piece_plus_a_byte_and_three_pieces_less_one(ctx, kind):
    """Multi-row parts whose spans are PIECE + 1 and 3 * PIECE - 1 bytes, behind parts of 0, 5 and 16 bytes: the
    destination of each starts at another alignment, and the windows are cut on the destination's grid."""
    rng = np.random.default_rng(kind + 1)

    def part(nbytes, rows):
        cuts = np.sort(rng.integers(0, nbytes + 1, rows - 1)) if rows > 1 else np.zeros(0, dtype=np.int64)
        edges = np.concatenate([[0], cuts, [nbytes]]).astype(np.int64)
        data = rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
        return [strings([data[a:b] for a, b in zip(edges[:-1], edges[1:])], kind, rng.random(rows) > 1 / 3, 1, lead=b"#" * 7)]

    for lead in (0, 5, 16):
        check(ctx, [part(lead, 2), part(PIECE + 1, 9), part(3 * PIECE - 1, 300), part(PIECE, 1), part(1, 1)])


# ---------------------------------------------------------------- 3. fixed width
@pytest.mark.parametrize("kind", [1, 4, 8])
def test_fixed_width_ranges_with_heads_and_tails_under_16_bytes(ctx, kind):
    rng = np.random.default_rng(kind)
    a, b = frame(rng, 300, [kind], 2), frame(rng, 41, [kind], 9)
    check(ctx, [a, b, a, b, a], [(1, 1), (3, 5), (1, 37), (5, 2), (7, 293)])       # `first` odd: sources off the 16-byte grid
    check(ctx, [a, b], [(1, 16 // kind + 1), (1, 3)])
    check(ctx, [a, b], [(3, 1), (0, 41)])
    n = PIECE // kind + 3                                                          # past one item
    big = frame(rng, n + 8, [kind], 0)
    check(ctx, [a, big, b], [(5, 1), (7, n), (0, 41)])


# ---------------------------------------------------------------- 4. grid and item edges
def test_past_one_round_of_every_grid_stride_launch(ctx):
    """The smallest frame past one round of each launch, in the device form (the host form runs the same kernels):
    four FIXED1 columns of 2^23 + 65 rows are CAP * 256 + 8 validity words and 4 * 513 > CAP copy items; the byte
    column's offsets are CAP + 1 rebase items and its 4-byte cells CAP + 1 copy items."""
    n = CAP * OFFSET_PIECE + 65
    assert 4 * -(-n // 64) > CAP * 256 and 4 * -(-n // PIECE) > CAP and -(-n // OFFSET_PIECE) > CAP and -(-4 * n // PIECE) > CAP
    rng = np.random.default_rng(11)
    cut = 4097

    def part(rows, bit):
        cols = [Column(1, rows, rng.integers(0, 256, rows, dtype=np.uint8), None, _rowhash.packed_at(rng.random(rows) > 0.5, bit + k, rng), 0, bit + k)
                for k in range(4)]
        offsets = (np.arange(rows + 1, dtype=np.int64) * 4 + 12).astype(np.int32)
        return cols + [Column(32, rows, rng.integers(0, 256, 4 * rows + 12, dtype=np.uint8), offsets, None)]

    parts = [part(cut + 3, 1), part(n - cut + 5, 6)]
    check(ctx, parts, [(3, cut), (2, n - cut)], forms=["device"])


# ---------------------------------------------------------------- 5. capacity
def test_sizes_only_and_a_capacity_one_byte_short(ctx):
    rng = np.random.default_rng(5)
    parts = [frame(rng, 50, [8, 32, 16, 64], 3), frame(rng, 9, [8, 32, 16, 64], 0)]
    ranges = [(4, 40), (0, 9)]
    want = _concat.concat(parts, ranges)
    sizes = sizes_of(want)
    need = [t.values.size for t in want]
    for form in FORMS:
        got = raw_call(ctx, form, parts, ranges, sizes, outputs=False)
        assert got.rc == OK and got.written == 0 and got.value_bytes == need, (form, got.err)
        assert_untouched(got, form)
        for short in (1, 3):
            capacity = list(need)
            capacity[short] -= 1
            got = raw_call(ctx, form, parts, ranges, sizes, capacity=capacity)
            assert got.rc == OK and got.written == 0 and got.value_bytes == need, (form, short, got.err)
            assert_untouched(got, (form, short))
        got = raw_call(ctx, form, parts, ranges, sizes, capacity=[0, need[1], 0, need[3] + 5])   # only the byte columns' room counts
        assert_same(got, want, form)


def test_bytes32_output_above_int32_offsets_is_refused(ctx):
    """Two parts alias one column of two cells of about 0.55 GiB each: 2.2 GiB, more than int32 offsets can say.
    Only the measure step runs -- the values are never read, so they need not be filled."""
    import torch

    cell = 590_000_000
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * cell + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the column alone needs {2 * cell >> 20}")
    values = torch.empty(2 * cell, dtype=torch.uint8, device="cuda:0")
    offsets = torch.tensor([0, cell, 2 * cell], dtype=torch.int32, device="cuda:0")
    col = Column(32, 2, values, offsets, None)
    outs = [torch.full((256,), SENTINEL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    head = tabular._concat_head([[col], [col]], [32], [2, 2], None, None, ptr)
    value_bytes, written = (ctypes.c_uint64 * 1)(7), ctypes.c_uint32(7)
    L = _capi.lib()
    for arrays, cap in (([None] * 3, None), ([tabular._pointers([o.data_ptr()]) for o in outs], (ctypes.c_uint64 * 1)(256))):
        rc = L.oxh_concat_columns_device(ctx.handle, *head, cap, *arrays, value_bytes, ctypes.byref(written), ctx.stream)
        assert rc == INVALID and b"OXH_COL_BYTES64" in L.oxh_last_error(), L.oxh_last_error()
        assert value_bytes[0] == 7 and written.value == 7
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    head = tabular._concat_head([[col], [col]], [32], [2, 2], [0, 1], [2, 1], ptr)          # three cells do fit
    rc = L.oxh_concat_columns_device(ctx.handle, *head, None, None, None, None, value_bytes, ctypes.byref(written), ctx.stream)
    assert rc == OK and value_bytes[0] == 3 * cell and written.value == 0


# ---------------------------------------------------------------- 6. bad offsets on the device
@pytest.mark.parametrize("kind", [32, 64])
def test_device_form_reads_a_bad_pair_as_a_cell_of_length_0(ctx, kind):
    """One decreasing pair and one negative start inside a taken range: the call finishes, returns
    OXH_ERR_INVALID, and the outputs are the restatement's "length 0" reading; the guards around every output
    hold. The host form refuses the same arguments and writes nothing."""
    rng = np.random.default_rng(kind)
    good = frame(rng, 40, [kind, 4], 1)
    dt = np.int32 if kind == 32 else np.int64
    decreasing = [good[0]._replace(offsets=np.array([3, 9, 6, 14, 20, 20, 31], dtype=dt), nrows=6, validity=None, validity_bit=0),
                  good[1]._replace(nrows=6)]
    negative = [good[0]._replace(offsets=np.array([4, -2, 5, 9], dtype=dt), nrows=3, validity=None, validity_bit=0), good[1]._replace(nrows=3)]
    for parts, ranges in (([good, decreasing, good], [(2, 5), (0, 6), (0, 20)]),
                          ([good, negative, good], [(2, 5), (1, 2), (0, 20)]),          # the part's span starts negative: nothing of it is read
                          ([good, negative, decreasing], [(0, 20), (0, 3), (1, 5)])):   # a negative offset inside a good span
        assert _concat.has_bad_offsets(parts, ranges)
        want = _concat.concat(parts, ranges, device_reading=True)
        got = raw_call(ctx, "device", parts, ranges, sizes_of(want))
        assert b"decrease or are negative" in got.err
        assert_same(got, want, ("device", ranges), rc=INVALID)
        got = raw_call(ctx, "host", parts, ranges, sizes_of(want))
        assert got.rc == INVALID and got.written == 7 and got.value_bytes == [7, 7]
        assert_untouched(got, "host")
    parts, ranges = [good, decreasing], [(0, 20), (3, 3)]                            # the bad pair is outside the taken range
    assert not _concat.has_bad_offsets(parts, ranges)
    check(ctx, parts, ranges)


# ---------------------------------------------------------------- 7. refusals and no rows
def test_refusals_leave_the_outputs_untouched_and_no_rows_is_ok(ctx):
    rng = np.random.default_rng(3)
    a, b = frame(rng, 10, [4, 32, 16], 0), frame(rng, 6, [4, 32, 16], 2)
    want = _concat.concat([a, b], [(1, 9), (0, 6)])
    sizes = sizes_of(want)
    for form in FORMS:
        for parts, ranges, what in (([a, b], [(1, 10), (0, 6)], b"part 0: first + count"),
                                    ([a, [b[0]._replace(kind=5), b[1], b[2]]], None, b"unknown kind"),
                                    ([a, [b[0], b[1]._replace(offsets=None), b[2]]], None, b"without offsets"),
                                    ([a, [b[0]._replace(values=None), b[1], b[2]]], None, b"has no values")):
            if what == b"unknown kind":
                parts = [[p[0]._replace(kind=5), p[1], p[2]] for p in parts]
            got = raw_call(ctx, form, parts, ranges, sizes)
            assert got.rc == INVALID and what in got.err, (form, what, got.err)
            assert got.written == 7 and got.value_bytes == [7, 7, 7]
            assert_untouched(got, (form, what))
        got = raw_call(ctx, form, [a, [b[0], b[1]._replace(values=None), b[2]]], [(1, 9), (0, 6)], sizes)   # bytes without values
        assert got.rc == INVALID and b"bytes but no values" in got.err, (form, got.err)
        assert_untouched(got, (form, "bytes without values"))
        # N == 0: OXH_OK with sizes 0; a byte column's single offset 0 is written, nothing else
        none = _concat.concat([a, b], [(3, 0), (6, 0)])
        assert [t.nrows for t in none] == [0, 0, 0] and none[1].offsets.tolist() == [0]
        assert_same(raw_call(ctx, form, [a, b], [(3, 0), (6, 0)], sizes_of(none)), none, (form, "no rows"))
        got = raw_call(ctx, form, [a, b], [(3, 0), (6, 0)], sizes_of(none), outputs=False)
        assert got.rc == OK and got.written == 0 and got.value_bytes == [0, 0, 0]
    L = _capi.lib()
    rc = L.oxh_concat_columns_host(None, 1, 1, (ctypes.c_uint32 * 1)(4), tabular._pointers([1]), tabular._pointers([None]),
                                   tabular._pointers([None]), (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 1)(1), None, None, None, None, None,
                                   None, (ctypes.c_uint64 * 1)(), ctypes.byref(ctypes.c_uint32()))
    assert rc == INVALID and b"ctx is NULL" in L.oxh_last_error()


# ---------------------------------------------------------------- 8. the Python layer, chains, the golden frame
def as_taken(c):
    """A Column the library returned (host arrays or device tensors), as the restatement's `Taken`."""
    host = lambda x: None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))  # noqa: E731
    values, offsets, validity = host(c.values), host(c.offsets), host(c.validity)
    return _take.Taken(int(c.kind), c.nrows, np.ascontiguousarray(values).view(np.uint8).reshape(-1), offsets, validity)


def assert_frames_equal(got, want, who):
    assert len(got) == len(want), who
    for k, (g, w) in enumerate(zip(got, want)):
        g = as_taken(g)
        assert (g.kind, g.nrows) == (w.kind, w.nrows), (who, k)
        assert np.array_equal(g.values, w.values) and np.array_equal(g.validity, w.validity), (who, k)
        assert (g.offsets is None) == (w.offsets is None) and (g.offsets is None or np.array_equal(g.offsets, w.offsets)), (who, k)
        assert g.offsets is None or g.offsets.dtype == w.offsets.dtype, (who, k)


def as_column(t):
    return Column(t.kind, t.nrows, t.values, t.offsets, t.validity, 0, 0)


def test_python_layer_both_forms(ctx):
    rng = np.random.default_rng(21)
    kinds = [8, 32, 16, 4, 64, 1]
    a, b = frame(rng, 33, kinds, 3), frame(rng, 70, kinds, 0)
    names = [f"c{k}" for k in range(len(kinds))]
    fa, fb = dict(zip(names, a)), dict(zip(names, b))
    cache = {}
    da, db = ({n: device_column(c, cache) for n, c in f.items()} for f in (fa, fb))
    want = _concat.concat([a, b, a], [(1, 30), (0, 70), (32, 1)])
    assert_frames_equal(tabular.concat([a, b, a], [(1, 30), (0, 70), (32, 1)], ctx=ctx), want, "concat")
    assert_frames_equal(tabular.concat_device([list(da.values()), list(db.values()), list(da.values())], [(1, 30), (0, 70), (32, 1)], ctx=ctx),
                        want, "concat_device")
    want = _concat.concat([a, b])
    got = tabular.vstack([fa, fb], ctx=ctx)
    assert list(got) == names
    assert_frames_equal(list(got.values()), want, "vstack")
    assert_frames_equal(list(tabular.vstack_device([da, db], ctx=ctx).values()), want, "vstack_device")
    assert got["c0"].values.dtype == a[0].values.dtype
    for call, dcall, args, rows in ((tabular.slice_rows, tabular.slice_rows_device, (5, 11), (5, 11)),
                                    (tabular.slice_rows, tabular.slice_rows_device, (-4, 9), (66, 4)),
                                    (tabular.slice_rows, tabular.slice_rows_device, (90, 9), (70, 0)),
                                    (tabular.head, tabular.head_device, (64,), (0, 64)), (tabular.head, tabular.head_device, (99,), (0, 70)),
                                    (tabular.tail, tabular.tail_device, (9,), (61, 9)), (tabular.tail, tabular.tail_device, (0,), (0, 0)),
                                    (tabular.page, tabular.page_device, (32, 3), (64, 6)), (tabular.page, tabular.page_device, (32, 0), (0, 32))):
        want = _concat.concat([b], [rows])
        assert_frames_equal(list(call(fb, *args, ctx=ctx).values()), want, (call.__name__, args))
        assert_frames_equal(list(dcall(db, *args, ctx=ctx).values()), want, (dcall.__name__, args))


def test_chains_on_the_device_equal_the_chains_of_the_restatements(ctx):
    """filter -> take -> slice / tail, and vstack of two frames -> unique: nothing but sizes crosses the link."""
    rng = np.random.default_rng(8)
    n = 500
    key = column(rng.integers(0, 40, n).astype(np.int64))
    text = strings([bytes(rng.integers(97, 100, int(l), dtype=np.uint8)) for l in rng.integers(0, 4, n)], 32, rng.random(n) > 0.2, 5, lead=b"..")
    flag = Column(16, n, _rowhash.packed_at(rng.random(n) > 0.5, 3, rng), None, _rowhash.packed_at(rng.random(n) > 0.1, 9, rng), 3, 9)
    cols = [key, text, flag]
    dev = [device_column(c) for c in cols]
    terms = [(0, F.GT, 10)]
    picked = F.filter_rows(cols, terms, (), [F.SIGNED] * 3)
    taken = [as_column(t) for t in _take.take(cols, picked.idx)]
    selected = tabular.filter_rows_device(dev, terms, ctx=ctx)
    dtaken = tabular.take_device(dev, selected.idx, ctx=ctx)
    names = ["key", "text", "flag"]
    m = taken[0].nrows
    assert m == selected.stats.selected and m > 120
    for got, rows in ((tabular.slice_rows_device(dict(zip(names, dtaken)), 100, 17, ctx=ctx), (100, 17)),
                      (tabular.tail_device(dict(zip(names, dtaken)), 65, ctx=ctx), (m - 65, 65))):
        assert_frames_equal(list(got.values()), _concat.concat([taken], [rows]), rows)
    # vstack -> unique on (key, flag): the take's canonical output in, canonical output out
    other = [as_column(t) for t in _take.take(cols, np.arange(n - 1, -1, -3, dtype=np.uint32))]
    dother = tabular.take_device(dev, tensor(np.arange(n - 1, -1, -3, dtype=np.int32)), ctx=ctx)
    stacked = [as_column(t) for t in _concat.concat([taken, other])]
    dstacked = list(tabular.vstack_device([dict(zip(names, dtaken)), dict(zip(names, dother))], ctx=ctx).values())
    assert_frames_equal(dstacked, _concat.concat([taken, other]), "vstack")
    groups = _grouprows.group_rows([stacked[0], stacked[2]])
    dgroups = tabular.group_rows_device([dstacked[0], dstacked[2]], ctx=ctx)
    assert dgroups.stats.groups == groups.stats[0]
    assert_frames_equal(tabular.take_device(dstacked, dgroups.first_idx, ctx=ctx), _take.take(stacked, groups.first_idx), "unique")


def test_vstack_and_slice_of_a_csv_fixture(ctx):
    """mixed_data_types.csv parsed into five columns (two strings, a boolean, a float, an integer): vstack of the frame
    with itself, then a slice across the seam -- the expected rows are the CSV's own, by list arithmetic."""
    with open(CSV, newline="") as f:
        header, *rows = list(csv.reader(f))
    assert header == ["prompt", "response", "is_correct", "response_time", "difficulty"] and len(rows) >= 3
    fr = {"prompt": column([r[0] for r in rows]), "response": column([r[1] for r in rows]),
          "is_correct": column(np.array([r[2] == "true" for r in rows])), "response_time": column(np.array([float(r[3]) for r in rows])),
          "difficulty": column(np.array([int(r[4]) for r in rows], dtype=np.int64))}
    n = len(rows)
    expect = (rows + rows)[n - 2:n + 3]
    for form in FORMS:
        if form == "host":
            got = tabular.slice_rows(tabular.vstack([fr, fr], ctx=ctx), n - 2, 5, ctx=ctx)
        else:
            d = {k: device_column(c) for k, c in fr.items()}
            got = tabular.slice_rows_device(tabular.vstack_device([d, d], ctx=ctx), n - 2, 5, ctx=ctx)
        got = {k: as_taken(c) for k, c in got.items()}
        assert list(got) == header
        assert _take.pylist(got["prompt"]) == [r[0] for r in expect] and _take.pylist(got["response"]) == [r[1] for r in expect]
        assert _take.pylist(got["is_correct"]) == [r[2] == "true" for r in expect]
        assert got["response_time"].values.view(np.float64).tolist() == [float(r[3]) for r in expect]
        assert got["difficulty"].values.view(np.int64).tolist() == [int(r[4]) for r in expect]
