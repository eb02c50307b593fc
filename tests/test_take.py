"""The take of the joined rows' columns on the GPU (oxh_take_columns_*, oxen_amd/csrc/take_columns.hip;
oxen_amd.tabular): every output buffer of both forms is compared, byte for byte, with the plain-numpy
restatement of tests/_take.py -- validity with zero pad bits, fixed-width values with zero under nulls,
bit-packed booleans, offsets from 0 in the column's own width, tightly packed bytes."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest

import _keyeddiff
import _rowhash
import _take
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
NONE = _capi.OXH_TAKE_NULL
VP = ctypes.c_void_p
SOURCE = open(os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc", "take_columns.hip")).read()
T = int(re.search(r"constexpr uint32_t kTakeShortMax = (\d+);", SOURCE).group(1))   # the shipped short / long threshold
P = int(re.search(r"constexpr uint32_t kTakePiece = (\d+);", SOURCE).group(1))      # and piece size


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


def device_index(a):
    return None if a is None else tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def as_taken(c):
    """A Column the Python layer returned (numpy or torch buffers) as a `_take.Taken` of numpy buffers."""
    host = lambda x: None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))  # noqa: E731
    assert c.value_bit == 0 and c.validity_bit == 0 and c.validity is not None
    return _take.Taken(c.kind, c.nrows, host(c.values).view(np.uint8).reshape(-1), host(c.offsets), host(c.validity))


def python_call(ctx, form, cols, i0, i1=None, plan=None):
    import torch

    if form == "host":
        return [as_taken(c) for c in tabular.take(cols, i0, i1, plan, ctx=ctx)]
    dev = [device_column(c) for c in cols]
    d0, d1 = device_index(i0), device_index(i1)
    torch.cuda.synchronize()
    out = tabular.take_device(dev, d0, d1, plan, stream=ctx.stream, ctx=ctx)
    assert all(c.validity.is_cuda and c.values.is_cuda for c in out)
    return [as_taken(c) for c in out]


def same(got, want):
    assert len(got) == len(want)
    for o, (g, w) in enumerate(zip(got, want)):
        assert g.kind == w.kind and g.nrows == w.nrows, o
        assert np.array_equal(g.validity, w.validity), ("validity", o, g.kind)
        if w.offsets is None:
            assert g.offsets is None
        else:
            assert g.offsets.dtype == w.offsets.dtype and np.array_equal(g.offsets, w.offsets), ("offsets", o, g.kind)
        if not np.array_equal(g.values, w.values):
            bad = int(np.nonzero(g.values[:w.values.size] != w.values[:g.values.size])[0][0]) if g.values.size == w.values.size else -1
            raise AssertionError(("values", o, g.kind, g.values.size, w.values.size, bad))


def check(ctx, form, cols, i0, i1=None, plan=None):
    want = _take.take(cols, i0, i1, plan)
    same(python_call(ctx, form, cols, i0, i1, plan), want)
    return want


def strings(cells, kind=_take.BYTES32, valid=None, bit=0, lead=b""):
    """A byte column from a list of bytes: `lead` bytes before the first cell (so offsets[0] != 0), the
    validity bitmap's row 0 at `bit`. A null cell keeps its bytes underneath, as Arrow allows."""
    off = np.zeros(len(cells) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cells], out=off[1:])
    data = np.frombuffer(lead + b"".join(cells), dtype=np.uint8)
    offsets = (off + len(lead)).astype(np.int32 if kind == _take.BYTES32 else np.int64)
    return Column(kind, len(cells), data, offsets, None if valid is None else _rowhash.packed_at(valid, bit), 0,
                  0 if valid is None else bit)


@functools.lru_cache(maxsize=None)
def frame(nrows, seed, bit=0):
    """All six kinds, each with nulls; the validity bitmaps and the boolean values start at bit `bit`, the
    BYTES32 column's offsets at 5. Empty strings and null strings with bytes underneath."""
    rng = np.random.default_rng(1000 * nrows + seed)
    valid = lambda: rng.random(nrows) > 0.2  # noqa: E731
    bitmap = lambda: _rowhash.packed_at(valid(), bit)  # noqa: E731
    words = [bytes(rng.integers(97, 123, size=int(l), dtype=np.uint8)) for l in rng.integers(0, 14, size=nrows)]
    return (
        Column(1, nrows, rng.integers(-128, 128, size=nrows).astype(np.int8), None, bitmap(), 0, bit),
        Column(4, nrows, rng.integers(-2**31, 2**31, size=nrows).astype(np.int32), None, bitmap(), 0, bit),
        Column(8, nrows, rng.integers(-2**63, 2**63, size=nrows).astype(np.int64), None, None, 0, 0),
        Column(16, nrows, _rowhash.packed_at(rng.random(nrows) < 0.5, bit), None, bitmap(), bit, bit),
        strings(words, _take.BYTES32, valid(), bit, lead=b"LEAD!"),
        strings(words[::-1], _take.BYTES64, valid(), bit),
    )


def indices(pattern, nout, nrows, rng):
    if pattern == "identity":
        return (np.arange(nout) % nrows).astype(np.uint32)
    if pattern == "reversed":
        return ((nrows - 1 - np.arange(nout)) % nrows).astype(np.uint32)
    i = rng.integers(0, nrows, size=nout).astype(np.uint32)   # random, with repeats
    if pattern == "all absent":
        i[:] = NONE
    if pattern == "every 3rd absent":
        i[::3] = NONE
    return i


def two_frame_plan(k):
    """Over a left frame's k columns then a right frame's: every left column through idx0, every right column
    through idx1, the right with the left as its fallback (the keys' coalesce), and the other way round."""
    return [(c, 0, None, 0) for c in range(k)] + [(k + c, 1, None, 0) for c in range(k)] + \
        [(k + c, 1, c, 0) for c in range(k)] + [(c, 0, k + c, 1) for c in range(k)]


# ---------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nout,nrows", list(itertools.product([0, 1, 63, 64, 65, 257], [1, 64, 257])) + [(70001, 70001)])
def test_sizes(ctx, form, nout, nrows):
    """From no output row to several workgroups, partial last bitmap words included; 70 001 rows also span
    several tiles of the scan (2 048 rows each) with a ragged tail."""
    rng = np.random.default_rng(nout * 1000 + nrows)
    left, right = frame(nrows, 1), frame(max(1, nrows - 3), 2)
    i0 = indices("every 3rd absent", nout, nrows, rng)
    i1 = indices("random", nout, max(1, nrows - 3), rng)
    i1[rng.random(nout) < 0.3] = NONE
    want = check(ctx, form, list(left) + list(right), i0, i1, two_frame_plan(len(left)))
    if nout >= 63 and nrows > 1:
        assert all(w.validity.any() for w in want) and not all(_rowhash.bits(w.validity, 0, nout).all() for w in want)


# ---------------------------------------------------------------- 2. index patterns
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pattern", ["identity", "reversed", "random", "all absent", "every 3rd absent", "idx0 None", "idx1 None"])
def test_index_patterns(ctx, form, pattern):
    rng = np.random.default_rng(11)
    left, right = frame(257, 3), frame(200, 4)
    nout = 300
    i0, i1 = indices(pattern, nout, 257, rng), indices("random", nout, 200, rng)
    if pattern == "idx0 None":
        i0 = None
    if pattern == "idx1 None":
        i1 = None
    want = check(ctx, form, list(left) + list(right), i0, i1, two_frame_plan(len(left)))
    if pattern in ("all absent", "idx0 None"):   # the plain takes of the left frame: all null, all zero
        assert all(not w.validity.any() and not w.values.any() for w in want[:6])
    if pattern == "identity":                    # the rows themselves (257 of them, then from row 0 again)
        assert _take.pylist(want[4], text=False)[:257] == _take.pylist(_take.take([left[4]], np.arange(257))[0], text=False)


# ---------------------------------------------------------------- 3. kinds and bit offsets
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bit", [0, 3, 13])
def test_every_kind_with_bitmaps_at_bit_offsets(ctx, form, bit):
    """Source validity and boolean values whose row 0 is at bit 0, 3, 13 (noise around them); a BYTES32
    source whose offsets[0] is 5; empty strings; null strings with bytes underneath."""
    rng = np.random.default_rng(bit)
    left, right = frame(131, 5, bit), frame(77, 6, (bit * 5) % 16)
    assert int(left[4].offsets[0]) == 5 and left[3].value_bit == bit and left[0].validity_bit == bit
    assert [c.kind for c in left] == [1, 4, 8, 16, 32, 64]
    i0, i1 = indices("every 3rd absent", 200, 131, rng), indices("random", 200, 77, rng)
    want = check(ctx, form, list(left) + list(right), i0, i1, two_frame_plan(6))
    cells = _take.pylist(want[4], text=False)
    assert b"" in cells and None in cells and any(c for c in cells)


# ---------------------------------------------------------------- 4. cell lengths
def aligned_cells():
    """Every length 0..17 at every destination alignment 0..7: before each cell a filler brings the output
    offset to the alignment wanted."""
    cells, at = [], 0
    for align in range(8):
        for length in range(18):
            pad = (align - at) % 8
            cells += [b"." * pad, bytes(range(65, 65 + length))]
            at += pad + length
    return cells


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", [_take.BYTES32, _take.BYTES64])
def test_short_cell_lengths_at_every_destination_alignment(ctx, form, kind):
    cells = aligned_cells()
    col = strings(cells, kind, lead=b"xyz")                      # the sources sit at other alignments than the places
    want = check(ctx, form, [col], np.arange(len(cells), dtype=np.uint32))
    assert want[0].values.tobytes() == b"".join(cells)
    starts = {(int(o) % 8, int(e - o)) for o, e in zip(want[0].offsets[:-1], want[0].offsets[1:])}
    assert {(a, n) for a in range(8) for n in range(18)} <= starts
    rng = np.random.default_rng(4)
    check(ctx, form, [col], rng.permutation(len(cells)).astype(np.uint32))


def threshold_cells(rng):
    """Cells of T - 1, T, T + 1 bytes around the short / long threshold and P - 1, P, P + 1, 2 P + 1 around the
    piece size, each among short cells (also the frame of tests/test_scratch_contents.py's take)."""
    body = lambda n: bytes(rng.integers(0, 256, size=n, dtype=np.uint8))  # noqa: E731
    cells = []
    for n in (T - 1, T, T + 1, P - 1, P, P + 1, 2 * P + 1):
        cells += [b"ab", body(n), b"c", b"", body(5)]
    return cells


@pytest.mark.parametrize("form", FORMS)
def test_cell_lengths_around_the_threshold_and_the_piece_size(ctx, form):
    """T - 1, T, T + 1 around the short / long threshold; P - 1, P, P + 1, 2 P + 1 around the piece size, each
    among short cells, at odd destinations; taken twice, in order and out of order."""
    rng = np.random.default_rng(8)
    body = lambda n: bytes(rng.integers(0, 256, size=n, dtype=np.uint8))  # noqa: E731
    cells = threshold_cells(rng)
    col = strings(cells, lead=b"q")
    order = np.arange(len(cells), dtype=np.uint32)
    want = check(ctx, form, [col], order)
    assert want[0].values.tobytes() == b"".join(cells)
    check(ctx, form, [col, strings(cells, _take.BYTES64)], order[::-1].copy(), order, [(0, 0, None, 0), (1, 1, None, 0), (1, 0, None, 0)])
    one = strings([b"s"] * 40 + [body(2 * P + 1)] + [b"t"] * 40)      # one such cell among short ones
    check(ctx, form, [one], np.concatenate([np.arange(81), [40, 40, NONE, 40]]).astype(np.uint32))


# ---------------------------------------------------------------- 5. fallback
@pytest.mark.parametrize("form", FORMS)
def test_fallback_rules(ctx, form):
    a = column(np.array([10, 11, 12, 13], dtype=np.int64), validity=[True, False, True, False])
    b = column(np.array([20, 21, 22], dtype=np.int64), validity=[True, True, False])
    sa, sb = column(["a0", None, "a2", None]), column(["b0", "b1", None])
    #                 primary:  present  null   absent  null   absent  present
    i0 = np.array([0, 1, NONE, 3, NONE, 2], dtype=np.uint32)
    #                 fallback: present  present present null  absent  absent
    i1 = np.array([1, 0, 1, 2, NONE, NONE], dtype=np.uint32)
    plan = [(0, 0, 1, 1), (2, 0, 3, 1), (1, 1, 0, 0), (3, 1, 2, 0), (0, 0, 0, 1), (0, 1, None, 0)]
    want = check(ctx, form, [a, b, sa, sb], i0, i1, plan)
    assert _take.pylist(want[0]) == [10, 20, 21, None, None, 12]            # primary, else fallback, else null
    assert _take.pylist(want[1]) == ["a0", "b0", "b1", None, None, "a2"]    # BYTES32 primary, BYTES32 fallback
    assert _take.pylist(want[2]) == [21, 20, 21, None, None, 12]            # the other way round
    assert _take.pylist(want[3]) == ["b1", "b0", "b1", None, None, "a2"]
    assert _take.pylist(want[4]) == [10, 10, None, 12, None, 12]            # the same column through the other index array
    assert _take.pylist(want[5]) == [None, 10, None, 12, None, None]        # a left column read through idx1
    assert want[1].offsets.tolist() == [0, 2, 4, 6, 6, 6, 8]


# ---------------------------------------------------------------- 6. capacity
def raw_call(ctx, form, cols, i0, i1, plan, capacity, sentinel=0xAB):
    """One call of the C entry. capacity: None for the sizes-only call (NULL output arrays), else the room of
    every output column's values; all output buffers are pre-filled with the sentinel. Returns (status code,
    value_bytes, written, [(values, offsets, validity) as uint8 arrays])."""
    import torch

    L = _capi.lib()
    nout_rows = len(i0 if i0 is not None else i1)
    rows, words, plan, kinds = tabular._take_tables(cols, plan)
    value_bytes = (ctypes.c_uint64 * len(plan))(*[7] * len(plan))
    written = ctypes.c_uint32(7)
    sizes = [] if capacity is None else tabular._take_sizes(kinds, nout_rows, capacity)
    outs = [[np.full(max(n, 8), sentinel, dtype=np.uint8) for n in size] for size in sizes]
    if form == "host":
        keep = []

        def ptr(a):
            if a is None:
                return None
            keep.append(np.ascontiguousarray(a))
            return keep[-1].ctypes.data if keep[-1].size else None

        tables = tabular._tables(cols, ptr)
        arrays = [None] * 4 if capacity is None else \
            [(ctypes.c_uint64 * len(plan))(*capacity)] + [tabular._pointers([o[k].ctypes.data for o in outs]) for k in range(3)]
        rc = L.oxh_take_columns_host(ctx.handle, len(cols), *tables, rows, nout_rows, ptr(i0), ptr(i1), len(plan), words, *arrays,
                                     value_bytes, ctypes.byref(written))
        return rc, list(value_bytes), written.value, outs
    dev = [device_column(c) for c in cols]
    d0, d1 = device_index(i0), device_index(i1)
    d_outs = [[tensor(a) for a in o] for o in outs]
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    arrays = [None] * 4 if capacity is None else \
        [(ctypes.c_uint64 * len(plan))(*capacity)] + [tabular._pointers([o[k].data_ptr() for o in d_outs]) for k in range(3)]
    rc = L.oxh_take_columns_device(ctx.handle, len(dev), *tabular._tables(dev, ptr), rows, nout_rows, ptr(d0), ptr(d1), len(plan),
                                   words, *arrays, value_bytes, ctypes.byref(written), ctx.stream)
    return rc, list(value_bytes), written.value, [[t.cpu().numpy() for t in o] for o in d_outs]


@pytest.mark.parametrize("form", FORMS)
def test_capacity_contract(ctx, form):
    rng = np.random.default_rng(21)
    cols = list(frame(257, 7))
    i0 = indices("every 3rd absent", 100, 257, rng)
    want = _take.take(cols, i0)
    need = [w.values.size for w in want]
    assert need[:4] == [100, 400, 800, 13] and need[4] > 0 and need[5] > 0
    rc, value_bytes, written, _ = raw_call(ctx, form, cols, i0, None, None, None)          # sizes only
    assert (rc, value_bytes, written) == (_capi.OXH_OK, need, 0)
    short = need[:5] + [need[5] - 1]                                                       # one byte too few in one column
    rc, value_bytes, written, outs = raw_call(ctx, form, cols, i0, None, None, short)
    assert (rc, value_bytes, written) == (_capi.OXH_OK, need, 0)
    assert all((a == 0xAB).all() for o in outs for a in o)                                 # nothing is touched
    rc, value_bytes, written, outs = raw_call(ctx, form, cols, i0, None, None, need)       # exactly enough
    assert (rc, value_bytes, written) == (_capi.OXH_OK, need, 1)
    more = [n + 9 for n in need]
    rc2, value_bytes2, written2, outs2 = raw_call(ctx, form, cols, i0, None, None, more)   # more: the rest stays
    assert (rc2, value_bytes2, written2) == (_capi.OXH_OK, need, 1)
    for w, o, o2 in zip(want, outs, outs2):
        nbits = (100 + 7) // 8
        for got in (o, o2):
            assert np.array_equal(got[0][:w.values.size], w.values) and np.array_equal(got[2][:nbits], w.validity)
            assert (got[2][nbits:] == 0xAB).all()
            if w.offsets is not None:
                assert np.array_equal(got[1][:w.offsets.nbytes], w.offsets.view(np.uint8)) and (got[1][w.offsets.nbytes:] == 0xAB).all()
        assert (o2[0][w.values.size:] == 0xAB).all() and o2[0].size >= w.values.size + 9


# ---------------------------------------------------------------- 7. what the device refuses
def test_bad_indices_and_offsets_on_the_device_form(ctx):
    cols = [column(np.arange(5, dtype=np.int64)), column(["ab", "cd", "ef", "g", ""])]
    ok = np.array([4, 0, NONE], dtype=np.uint32)
    rc, *_ = raw_call(ctx, "device", cols, ok, None, None, [24, 8])
    assert rc == _capi.OXH_OK
    bad = np.array([4, 5, NONE], dtype=np.uint32)                       # an index equal to src_rows
    for capacity in (None, [24, 8]):
        rc, value_bytes, written, _ = raw_call(ctx, "device", cols, bad, None, None, capacity)
        assert rc == _capi.OXH_ERR_INVALID and b"index" in _capi.lib().oxh_last_error()
        assert value_bytes == [7, 7] and written == 7
    rc, *_ = raw_call(ctx, "device", cols[:1], bad, None, None, [24])   # without a byte column there is no measure pass
    assert rc == _capi.OXH_ERR_INVALID and b"index" in _capi.lib().oxh_last_error()
    rc, *_ = raw_call(ctx, "host", cols, bad, None, None, [24, 8])      # the host form runs the same kernels
    assert rc == _capi.OXH_ERR_INVALID
    broken = cols[1]._replace(offsets=np.array([0, 2, 4, 3, 7, 7], dtype=np.int32))   # a decreasing pair at row 2
    rc, value_bytes, written, outs = raw_call(ctx, "device", [cols[0], broken], np.array([0, 1, 2, 3], dtype=np.uint32), None, None, [32, 16])
    assert rc == _capi.OXH_ERR_INVALID and b"offsets" in _capi.lib().oxh_last_error()
    assert all((a == 0xAB).all() for o in outs for a in o) and written == 7
    rc, *_ = raw_call(ctx, "device", [cols[0], broken], np.array([0, 1, 3, 4], dtype=np.uint32), None, None, [32, 16])
    assert rc == _capi.OXH_OK                                           # the pair is not among the rows taken


def test_a_bytes32_output_past_int32_says_to_pass_bytes64(ctx):
    """More than 2^31 - 1 output bytes from int32 offsets: 9 takes of one 256 MiB cell. Nothing is written."""
    import torch

    cell = 1 << 28
    values = torch.zeros(cell, dtype=torch.uint8, device="cuda:0")
    offsets = torch.tensor([0, cell], dtype=torch.int32, device="cuda:0")
    col = Column(_take.BYTES32, 1, values, offsets)
    idx = torch.zeros(9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(_capi.OxenError, match="OXH_COL_BYTES64") as e:
        tabular.take_device([col], idx, stream=ctx.stream, ctx=ctx)
    assert e.value.code == _capi.OXH_ERR_INVALID
    out = tabular.take_device([col], idx[:7], stream=ctx.stream, ctx=ctx)[0]      # 7 fit: 1.75 GiB
    assert out.offsets.cpu().tolist() == [k * cell for k in range(8)] and out.values.numel() == 7 * cell


# ---------------------------------------------------------------- 8. end to end
@functools.lru_cache(maxsize=None)
def two_frames():
    """The two frames of test_keyed_diff.py::test_diff_dfs_over_two_frames."""
    n = 500
    rng = np.random.default_rng(9)
    ids = rng.permutation(2 * n)[:n].astype(np.int64)
    id_valid = rng.random(n) > 0.03
    names = ["k%d" % (i % 211) for i in range(n)]
    score = rng.standard_normal(n)
    note = [None if i % 17 == 0 else "n%d" % (i % 5) for i in range(n)]
    left = {"id": column(ids, validity=id_valid), "name": column(names), "score": column(score), "note": column(note),
            "old": column(np.arange(n, dtype=np.int32))}
    keep = rng.permutation(n)[: n - 40]
    r_ids, r_valid = ids[keep].copy(), id_valid[keep].copy()
    r_names = [names[i] for i in keep]
    r_score, r_note = score[keep].copy(), [note[i] for i in keep]
    r_score[rng.random(keep.size) < 0.1] += 1.0
    r_note[3], r_note[4] = "changed", None
    r_valid[[10, 11]] = False
    extra = 30
    right = {"id": column(np.concatenate([r_ids, 5000 + np.arange(extra)]), validity=np.concatenate([r_valid, np.ones(extra, bool)])),
             "name": column(r_names + ["new%d" % i for i in range(extra)]),
             "score": column(np.concatenate([r_score, np.zeros(extra)])), "note": column(r_note + ["x"] * extra),
             "new": column(np.ones(keep.size + extra, dtype=bool))}
    return left, right


def restated_pairs(oracle_lib, left, right, keys, targets, key0):
    on = lambda f, names: _rowhash.row_hashes([c for k, c in f.items() if k in names], oracle_lib)  # noqa: E731
    rows = lambda t: None if t is None else [tuple(r) for r in np.asarray(t).tolist()]  # noqa: E731
    valid = lambda c: None if c.validity is None else _rowhash.bits(c.validity, c.validity_bit, c.nrows).tolist()  # noqa: E731
    lt = on(left, targets) if any(t in left for t in targets) else None
    rt = on(right, targets) if any(t in right for t in targets) else None
    pairs, _, _ = _keyeddiff.keyed_diff(rows(on(left, keys)), rows(on(right, keys)), rows(lt), rows(rt), valid(left[key0]),
                                        valid(right[key0]))
    side = lambda k: np.array([NONE if p[k] is None else p[k] for p in pairs], dtype=np.uint32)  # noqa: E731
    return side(0), side(1), [p[2] for p in pairs]


ARROW_TYPES = {"id": "int64", "name": "string", "score": "float64", "note": "string", "old": "int32", "new": "bool_"}


def test_diff_dfs_contents_over_two_frames(ctx, oracle_lib):
    """`diff_dfs_contents` end to end: every column of the contents against the restatement's take of the
    restated pairs, and -- where pyarrow imports -- its values against pyarrow's take / coalesce."""
    left, right = two_frames()
    sources = list(left.values()) + list(right.values())
    where = {("left", n): i for i, n in enumerate(left)}
    where.update({("right", n): len(left) + i for i, n in enumerate(right)})
    try:
        import pyarrow as pa
        import pyarrow.compute as pc
    except ImportError:
        pa = None
    for keys, targets, want_keys, want_targets, names in (
            (["id", "name"], ["score", "note"], ["id", "name"], ["score", "note"],
             ["id", "name", "score.left", "score.right", "note.left", "note.right"]),
            (["name", "id"], [], ["id", "name"], ["score", "note"],
             ["id", "name", "score.left", "score.right", "note.left", "note.right"]),
            ([], [], ["id", "name", "score", "note"], ["new", "old"], ["id", "name", "score", "note", "new.right"])):
        l, r, status = restated_pairs(oracle_lib, left, right, want_keys, want_targets, keys[0] if keys else "id")
        d, contents = tabular.diff_dfs_contents(left, right, keys=keys, targets=targets, ctx=ctx)
        assert list(contents) == names + ["_oxen_diff_status"]
        assert np.array_equal(np.where(d.left_rows < 0, NONE, d.left_rows), l) and d.status.tolist() == status and len(l) > 60
        assert np.array_equal(np.where(d.right_rows < 0, NONE, d.right_rows), r)
        assert _take.pylist(contents["_oxen_diff_status"]) == [tabular.STATUS_NAMES[s] for s in status]
        for name in names:
            stem, _, suffix = name.partition(".")
            if not suffix:    # a key: coalesce(right, left)
                entry = (where[("right", stem)], 1, where[("left", stem)], 0)
            else:
                entry = (where[(suffix, stem)], 0 if suffix == "left" else 1, None, 0)
            want = _take.take(sources, l, r, [entry])
            same([as_taken(contents[name])], want)
            if pa is not None:
                typ = getattr(pa, ARROW_TYPES[stem])()
                as_index = lambda i: pa.array([None if v == NONE else int(v) for v in i], type=pa.uint32())  # noqa: E731
                arrow = lambda f: tabular.columns_to_arrow({stem: f[stem]}, pa.schema([(stem, typ)])).column(0).combine_chunks()  # noqa: E731
                if not suffix:
                    theirs = pc.coalesce(arrow(right).take(as_index(r)), arrow(left).take(as_index(l)))
                else:
                    theirs = arrow(left).take(as_index(l)) if suffix == "left" else arrow(right).take(as_index(r))
                ours = tabular.columns_to_arrow({stem: contents[name]}, pa.schema([(stem, typ)])).column(0)
                assert ours.to_pylist() == theirs.to_pylist(), name
    # the keys are never null where either side has the row's key
    assert _rowhash.bits(contents["name"].validity, 0, contents["name"].nrows).all()


def test_take_device_straight_from_the_keyed_diff(ctx, oracle_lib):
    """The device chain with no host copy: row hashes, `keyed_diff_digests_device`, and `take_device` fed by
    its tensors as they are. The device diff may write the right rows of one left row in any order, so each
    run of equal left index is compared as a set of rows; the frames here have unique keys, so that is the
    row itself."""
    import torch

    left, right = two_frames()
    dl = {n: device_column(c) for n, c in left.items()}
    dr = {n: device_column(c) for n, c in right.items()}
    torch.cuda.synchronize()
    on = lambda f, names: tabular.row_hashes_device([c for k, c in f.items() if k in names], stream=ctx.stream, ctx=ctx)  # noqa: E731
    keys, targets = ["id", "name"], ["score", "note"]
    d = tabular.keyed_diff_digests_device(on(dl, keys), on(dr, keys), on(dl, targets), on(dr, targets),
                                          (dl["id"].validity, 0), (dr["id"].validity, 0), stream=ctx.stream, ctx=ctx)
    assert d.left_rows.is_cuda and d.left_rows.dtype == torch.int32
    wanted = tabular.output_columns(left, right, keys, targets)
    sources = list(dl.values()) + list(dr.values())
    where = {("left", n): i for i, n in enumerate(left)}
    where.update({("right", n): len(left) + i for i, n in enumerate(right)})
    side = {"left": 0, "right": 1}
    plan = [(where[a], side[a[0]], None if b is None else where[b], 0 if b is None else side[b[0]]) for _, a, b in wanted]
    got = tabular.take_device(sources, d.left_rows, d.right_rows, plan, stream=ctx.stream, ctx=ctx)
    assert all(c.values.is_cuda for c in got) and [w[0] for w in wanted] == ["id", "name", "score.left", "score.right", "note.left", "note.right"]
    l, r, status = restated_pairs(oracle_lib, left, right, keys, targets, "id")
    got_l, got_r = d.left_rows.cpu().numpy().view(np.uint32), d.right_rows.cpu().numpy().view(np.uint32)
    want = _take.take(list(left.values()) + list(right.values()), l, r, plan)
    # runs of equal left index: the same set of (left, right) rows, then the same cells row by row
    assert sorted(zip(got_l.tolist(), got_r.tolist())) == sorted(zip(l.tolist(), r.tolist()))
    order_got = np.lexsort((got_r, got_l))
    order_want = np.lexsort((r, l))
    assert np.array_equal(got_l[order_got], l[order_want])
    for g, w in zip(got, want):
        cells_g, cells_w = _take.pylist(as_taken(g), text=False), _take.pylist(w, text=False)
        assert [cells_g[i] for i in order_got] == [cells_w[i] for i in order_want]
    if np.array_equal(got_l, l) and np.array_equal(got_r, r):   # the same order (unique keys): then byte for byte
        same([as_taken(g) for g in got], want)


# ---------------------------------------------------------------- 9. repeatability
def test_the_same_call_twice_and_the_contexts_own_index(ctx):
    from oxen_amd.dedup import DedupIndex

    rng = np.random.default_rng(33)
    left, right = frame(257, 8), frame(200, 9)
    cols = list(left) + list(right)
    cells = [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (T + 5, 3, 2 * P + 9, 0, P)] * 4
    cols.append(strings(cells))                                           # long cells too: the item lists' order is not fixed
    plan = two_frame_plan(6) + [(12, 0, None, 0)]
    i0, i1 = indices("every 3rd absent", 300, 20, rng), indices("random", 300, 200, rng)
    mine = np.stack([np.arange(1000, dtype=np.uint64) % 600 + 7, np.arange(1000, dtype=np.uint64) % 600], axis=1)
    with DedupIndex(ctx) as index:
        first, _ = index.insert(mine)
        before = index.counts()
        for form in FORMS:
            a = python_call(ctx, form, cols, i0, i1, plan)
            b = python_call(ctx, form, cols, i0, i1, plan)
            same(a, b)
            same(a, _take.take(cols, i0, i1, plan))
        assert index.counts() == before                                   # the context's own index is what it was
        assert np.array_equal(index.query(mine), first)
