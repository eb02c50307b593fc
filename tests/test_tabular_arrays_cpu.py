"""The array restatements of tests/_tabular_arrays.py pinned to their plain-Python originals
(`_sortrows.sort_indices`, `_keyeddiff.keyed_diff`, `_rowhash.compute_new_row_indices`) with exact equality,
over the generators the GPU cases of tests/test_tabular_past_grid.py use, at small row counts; and the
structure those generators plant around an edge, checked at a small edge. No GPU."""
import numpy as np
import pytest

import _keyeddiff
import _rowhash
import _sortrows
import _tabular_arrays as ta
import _take
from _tabular_arrays import SIGNED, UNSIGNED
from oxen_amd.tabular import Column

ROWS = [0, 1, 2, 257, 5000]


# ---------------------------------------------------------------- sort
def same_sort(cols, orders=None):
    want, tied = _sortrows.sort_indices(cols, orders)
    got, got_tied = ta.sort_indices_arrays(cols, orders)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want) and got_tied == tied
    return got, tied


@pytest.mark.parametrize("n", ROWS)
def test_sort_of_integer_keys(n):
    keys = ta.int64_keys(n)
    perm, tied = same_sort([Column(8, n, keys)])
    assert tied == 0
    if n:
        assert np.array_equal(perm, np.argsort(keys, kind="stable"))       # what E1 compares with
    same_sort([Column(8, n, keys)], [UNSIGNED])                             # -1 is then the largest key
    same_sort([ta.with_nulls(Column(8, n, keys), n)])
    rng = np.random.default_rng(n)
    few = keys[rng.integers(0, min(n, 5), size=n)] if n else keys           # duplicate values, the extremes among them
    perm, tied = same_sort([Column(8, n, few)])
    assert tied == (n if n > 100 else tied)
    same_sort([ta.with_nulls(Column(8, n, few), n + 1)], [UNSIGNED])
    for dtype, order in ((np.int8, SIGNED), (np.uint8, UNSIGNED), (np.int32, SIGNED), (np.uint32, UNSIGNED), (np.uint64, UNSIGNED)):
        info = np.iinfo(dtype)
        v = np.concatenate([np.array([info.min, info.max], dtype=dtype), rng.integers(info.min, int(info.max) + 1, size=n, dtype=dtype)])[:n]
        same_sort([ta.with_nulls(Column(v.dtype.itemsize, n, v), n + 2, bit=3)], [order])


@pytest.mark.parametrize("n", ROWS)
def test_sort_of_two_keys_with_nulls_in_the_first(n):
    first, second = ta.grouped_keys(n, distinct=max(1, n // 40))
    perm, tied = same_sort([first, second])
    if n > 100:
        valid = _rowhash.bits(first.validity, 5, n)
        nulls = int((~valid).sum())
        assert n // 4 < nulls < n // 2 and not valid[perm[:nulls]].any() and valid[perm[nulls:]].all()
    same_sort([first])                                                       # alone: many ties, in input order
    same_sort([second, first])


@pytest.mark.parametrize("n", [1, 2, 257, 5000])
def test_sort_of_one_row_that_differs(n):
    for byte in (0, 3, 7):
        perm, tied = same_sort([Column(8, n, ta.one_low_row(n, byte))])
        assert perm.tolist() == [n - 1] + list(range(n - 1)) and tied == (n - 1 if n > 2 else 0)
    for col in (ta.one_null_row(n), ta.one_short_row(n)):
        perm, tied = same_sort([col])
        assert perm.tolist() == [n - 1] + list(range(n - 1))
    assert _sortrows.cells(ta.one_short_row(3)) == [(1, b"abc"), (1, b"abc"), (1, b"ab")]
    assert _sortrows.cells(ta.one_null_row(3)) == [(1, ta.EQUAL_KEY), (1, ta.EQUAL_KEY), (0,)]


@pytest.mark.parametrize("n", ROWS)
def test_sort_of_short_byte_cells(n):
    """Cells of 0, 7, 8, 9, 15 and 16 bytes and cells that differ only by trailing zero bytes."""
    cells = ta.short_cells(n)
    if n >= 257:
        assert {len(c) for c in cells} >= {0, 7, 8, 9, 15, 16} and {b"a", b"a\0", b"a\0\0"} <= set(cells)
    col = ta.cells_column(cells)
    perm, tied = same_sort([col])
    assert tied == (n if n >= 5000 else tied)
    same_sort([ta.with_nulls(col, n, bit=5)])
    same_sort([ta.cells_column(cells, _take.BYTES64), Column(8, n, ta.int64_keys(n))])
    # the ladder alone, every cell once: a proper prefix first, a zero byte below every other byte
    ladder = ta.cells_column(ta.LADDER)
    perm, tied = same_sort([ladder])
    assert tied == 0 and [ta.LADDER[i] for i in perm] == sorted(ta.LADDER)


# ---------------------------------------------------------------- keyed diff
def as_pairs(arrays):
    lrows, rrows, status = arrays
    side = lambda a: [None if v < 0 else v for v in a.tolist()]  # noqa: E731
    return list(zip(side(lrows), side(rrows), status.tolist()))


@pytest.mark.parametrize("keep", [False, True], ids=["changed", "all"])
@pytest.mark.parametrize("nl,nr", [(a, b) for a in ROWS for b in ROWS if abs(a - b) < 4000] + [(5000, 5047), (257, 2305)])
def test_keyed_diff_of_unique_integer_keys(nl, nr, keep):
    left, right, lt, rt = ta.keyed_int_case(nl, nr)
    for tl, tr in ((lt, rt), (None, rt), (lt, None), (None, None)):
        want = _keyeddiff.keyed_diff(left.tolist(), right.tolist(), None if tl is None else tl.tolist(),
                                     None if tr is None else tr.tolist(), keep_unchanged=keep)
        arrays, counts, dupes = ta.keyed_diff_arrays(left, right, tl, tr, keep)
        assert (as_pairs(arrays), counts, dupes) == want
    if min(nl, nr) >= 257:
        _, counts, _ = ta.keyed_diff_arrays(left, right, lt, rt, keep)
        small = min(nl, nr)
        assert all(small // 10 < counts[s] for s in (_keyeddiff.ADDED, _keyeddiff.REMOVED, _keyeddiff.MODIFIED))   # about a fifth each
        assert counts[_keyeddiff.UNCHANGED] > small // 2


# ---------------------------------------------------------------- row diff
@pytest.mark.parametrize("nbase,nhead", [(a, b) for a in ROWS for b in ROWS] + [(259, 387), (5003, 5131)])
def test_row_diff_flags(nbase, nhead):
    base, head = ta.row_diff_keys(nbase, nhead, tail=min(300, nbase // 4))
    removed, added, counts = ta.row_diff_arrays(base, head)
    want_added, want_removed = _rowhash.compute_new_row_indices(base.tolist(), head.tolist())
    assert np.nonzero(added)[0].tolist() == want_added and np.nonzero(removed)[0].tolist() == want_removed
    assert counts == (len(want_removed), len(want_added)) and removed.dtype == added.dtype == np.uint8


def test_row_diff_of_repeated_keys():
    # key 5 is three times in base and not in head; key 9 twice in head and not in base; 1 and 2 in both
    removed, added, counts = ta.row_diff_arrays([5, 1, 5, 2, 5, 1], [9, 1, 2, 9, 2])
    assert removed.tolist() == [0, 0, 0, 0, 1, 0] and added.tolist() == [0, 0, 0, 1, 0] and counts == (1, 1)


# ---------------------------------------------------------------- the planted structure, at a small edge
EDGE = 512


def test_planted_rows_of_the_hash_frames():
    cols = ta.hash_frame(EDGE + 257, [(5, 300), (EDGE + 5, 421)])
    lens = _rowhash.assemble(cols)[2].astype(np.int64)
    assert lens.size == EDGE + 257 and lens[5] == 300 and lens[EDGE + 5] == 421
    rest = np.delete(lens, [5, EDGE + 5])
    assert rest.min() == 4 and rest.max() == 12                 # every other row is short, whatever LDS slot the call picks
    assert np.nonzero(lens > 12)[0].tolist() == [5, EDGE + 5]
    assert (_rowhash.assemble(ta.hash_frame(EDGE + 257))[2] <= 12).all()


def test_planted_rows_of_the_row_diff():
    nbase, nhead, tail = EDGE // 2 + 3, EDGE // 2 + 131, 40
    base, head = ta.row_diff_keys(nbase, nhead, tail)
    removed, added, counts = ta.row_diff_arrays(base, head)
    assert base.size == nbase and head.size == nhead
    assert removed[-tail:].all() and added[-tail:].all()         # every one of the last rows of either side is flagged
    ordinals = nbase + np.nonzero(added)[0]                       # a head row's place among all rows of the call
    assert (ordinals >= EDGE).sum() >= 40 and (ordinals < EDGE).any()
    assert counts[0] > tail and np.unique(base).size < nbase      # changed rows and repeats beside the planted ones


def test_planted_groups_of_the_keyed_diff():
    nl, nr = 67, EDGE + 257
    left, right, lt, rt, groups = ta.dupes_split_case(nl, nr, EDGE)
    assert left.size == nl and right.size == nr and len(groups) == 7
    for kind, (a, b), key, rows in groups:
        assert np.array_equal(np.nonzero(right == key)[0], rows) and rows.size == b and (left == key).sum() == a
        if kind == "past":
            assert rows.min() >= EDGE and (np.diff(rows) == 1).all()   # a run of neighbours past the edge
        else:
            assert rows.min() < EDGE <= rows.max()
    assert [m for k, m, _, _ in groups if k == "past"] == [(1, 2), (2, 3), (1, 65)]
    assert [m for k, m, _, _ in groups if k == "split"] == [(1, 2), (2, 3), (1, 65), (1, 300)]
    two = next(rows for k, m, _, rows in groups if k == "split" and m == (1, 2))
    assert two.tolist() == [EDGE - 1, EDGE]                       # equal neighbours, one on each side
    pairs, counts, dupes = _keyeddiff.keyed_diff(left.tolist(), right.tolist(), lt.tolist(), rt.tolist(), keep_unchanged=True)
    assert dupes == (2 * 2, 2 * (2 + 3 + 65) + 300)
    assert all(counts[s] for s in counts) and len(pairs) == sum(counts.values()) > nr
    # outside the groups every key is unique
    values, times = np.unique(np.concatenate([left, right + 0]), return_counts=True)
    assert set(values[times > 2].tolist()) <= {key for _, _, key, _ in groups}


def test_planted_cells_of_the_take():
    cols, idx0, idx1, plan = ta.take_case(EDGE + 1, big_at=(0, EDGE), nrows=300)
    assert [c.kind for c in cols] == [8, 32, 16, 8, 32, 16] and cols[0].nrows == 300 and cols[3].nrows == 297
    out = _take.take(cols, idx0, idx1, plan)
    lens = np.diff(out[1].offsets.astype(np.int64))
    assert lens[0] == lens[EDGE] == ta.BIG_CELL and np.delete(lens, [0, EDGE]).max() == 7
    assert int(out[1].offsets[-1]) == lens.sum() > 2 * ta.BIG_CELL
    absent = (idx0 == ta.NONE).mean()
    assert 1 / 16 < absent < 3 / 16 and 1 / 16 < (idx1 == ta.NONE).mean() < 3 / 16
    for t in out:                                                  # nulls, fallbacks and primaries in every column
        valid = _take.bits(t.validity, 0, t.nrows)
        assert valid.any() and not valid.all()
    primary = _take.take(cols, idx0, idx1, [(c, 0, None, 0) for c in range(3)])
    assert any(not np.array_equal(p.validity, t.validity) for p, t in zip(primary, out))
