"""The keyed tabular diff on the GPU (oxh_keyed_diff_*, oxen_amd/csrc/keyed_diff.hip; oxen_amd.tabular):
every result is compared, exactly, with the plain-Python restatement of tests/_keyeddiff.py, through both
the host and the device form. The host form's pairs are compared as they come; the device form may write
the right rows of one left row in any order, so each run of equal left index is first checked to hold the
right set, then sorted. The status rule is restated from join_diff.rs:458-484, not pinned by a run of
polars."""
import functools
import itertools

import numpy as np
import pytest

import _keyeddiff
import _rowhash
from oxen_amd import _capi, tabular
from oxen_amd.tabular import column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
NONE = _capi.OXH_KEYED_DIFF_NONE
U, A, R, M = _keyeddiff.UNCHANGED, _keyeddiff.ADDED, _keyeddiff.REMOVED, _keyeddiff.MODIFIED


def digests_of(keys):
    """(n, 2) digests that are equal exactly where the integer keys are."""
    k = np.asarray(keys, dtype=np.uint64).reshape(-1)
    return np.stack([k * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1), k ^ np.uint64(0xC2B2AE3D27D4EB4F)], axis=1)


def rows_of(table):
    return None if table is None else [tuple(r) for r in np.asarray(table, dtype=np.uint64).reshape(-1, 2).tolist()]


def on_device(a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(signed).copy()).to("cuda:0")


class Case:
    """The inputs of one call: digest tables (targets may be None) and the validity of keys[0] per side as
    (boolean mask or None, bit of row 0 in the bitmap the call gets)."""

    def __init__(self, lk, rk, lt=None, rt=None, lvalid=None, rvalid=None, lbit=0, rbit=0):
        self.lk, self.rk, self.lt, self.rt = lk, rk, lt, rt
        self.lvalid, self.rvalid, self.lbit, self.rbit = lvalid, rvalid, lbit, rbit
        self.nl, self.nr = lk.shape[0], rk.shape[0]
        self.lmap = None if lvalid is None else _rowhash.packed_at(lvalid, lbit)
        self.rmap = None if rvalid is None else _rowhash.packed_at(rvalid, rbit)

    @functools.lru_cache(maxsize=None)
    def want(self, keep):
        return _keyeddiff.keyed_diff(rows_of(self.lk), rows_of(self.rk), rows_of(self.lt), rows_of(self.rt),
                                     None if self.lvalid is None else list(self.lvalid),
                                     None if self.rvalid is None else list(self.rvalid), keep)


def triples(left, right, status):
    side = lambda a: [None if v == NONE else v for v in np.asarray(a).view(np.uint32).tolist()]  # noqa: E731
    return list(zip(side(left), side(right), np.asarray(status).tolist()))


def runs(pairs):
    """The pairs cut into the runs of one left row; every right-only row is a run of its own."""
    out = []
    for p in pairs:
        if out and p[0] is not None and out[-1][0][0] == p[0]:
            out[-1].append(p)
        else:
            out.append([p])
    return out


def ordered(form, got, want):
    """`got` with the right rows ascending inside each left row's pairs, after checking -- for the device form,
    which may write them in any order -- that each such run holds the set `want` has there."""
    if form == "host":
        return got
    got_runs, want_runs = runs(got), runs(want)
    assert [r[0][0] for r in got_runs] == [r[0][0] for r in want_runs]
    for g, w in zip(got_runs, want_runs):
        assert sorted(g, key=lambda p: -1 if p[1] is None else p[1]) == w, (g[:4], w[:4])
    return [p for r in got_runs for p in sorted(r, key=lambda p: -1 if p[1] is None else p[1])]


def python_call(ctx, form, case, keep=False):
    """The result through the Python layer of one form: (pairs, KeyedDiff)."""
    import torch

    lv = None if case.lmap is None else (case.lmap, case.lbit)
    rv = None if case.rmap is None else (case.rmap, case.rbit)
    if form == "host":
        d = tabular.keyed_diff_digests(case.lk, case.rk, case.lt, case.rt, lv, rv, keep_unchanged=keep, ctx=ctx)
        assert d.left_rows.dtype == np.int64 and d.right_rows.dtype == np.int64 and d.status.dtype == np.uint8
        pairs = [(None if l < 0 else l, None if r < 0 else r, s)
                 for l, r, s in zip(d.left_rows.tolist(), d.right_rows.tolist(), d.status.tolist())]
        return pairs, d
    dev = [on_device(t) for t in (case.lk, case.rk, case.lt, case.rt)]
    dlv = None if lv is None else (on_device(lv[0]), lv[1])
    drv = None if rv is None else (on_device(rv[0]), rv[1])
    torch.cuda.synchronize()
    d = tabular.keyed_diff_digests_device(*dev, dlv, drv, keep_unchanged=keep, stream=ctx.stream, ctx=ctx)
    assert d.left_rows.dtype == torch.int32 and d.status.dtype == torch.uint8 and d.left_rows.is_cuda
    return triples(d.left_rows.cpu().numpy(), d.right_rows.cpu().numpy(), d.status.cpu().numpy()), d


def check(ctx, form, case, keep=False):
    want, counts, dupes = case.want(keep)
    pairs, d = python_call(ctx, form, case, keep)
    assert (d.added, d.removed, d.modified, d.unchanged) == (counts[A], counts[R], counts[M], counts[U])
    assert (d.dupes_left, d.dupes_right) == dupes
    assert len(pairs) == len(want)
    got = ordered(form, pairs, want)
    if got != want:
        bad = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
        raise AssertionError((bad, got[bad:bad + 4], want[bad:bad + 4]))
    return want, counts, dupes


def raw_call(ctx, form, case, flags, capacity, sentinel=0xAB):
    """One call of the C entry with output arrays of max(capacity, 1) entries pre-filled with a sentinel
    (NULL arrays when capacity is None: the counts-only call): (status code, counts8, left, right, status)."""
    import torch

    L = _capi.lib()
    counts = np.full(8, 7, dtype=np.uint64)
    bits = np.array([case.lbit, case.rbit], dtype=np.uint64)
    size = max(capacity or 0, 1)
    left = np.full(size, sentinel * 0x01010101, dtype=np.uint32)
    right, status = left.copy(), np.full(size, sentinel, dtype=np.uint8)
    tables = [case.lk, case.rk, case.lt, case.rt, case.lmap, case.rmap]
    cp, bp = counts.ctypes.data_as(_capi._u64p), bits.ctypes.data_as(_capi._u64p)
    if form == "host":
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        lk, rk, lt, rt, lv, rv = [ptr(t) for t in tables]
        outs = [None] * 3 if capacity is None else [left.ctypes.data, right.ctypes.data, status.ctypes.data]
        rc = L.oxh_keyed_diff_host(ctx.handle, lk, case.nl, rk, case.nr, lt, rt, lv, rv, bp, flags, capacity or 0, *outs, cp)
        return rc, counts.tolist(), left, right, status
    dev = [on_device(t) for t in tables]
    d_out = [on_device(a) for a in (left, right, status)]
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    lk, rk, lt, rt, lv, rv = [ptr(t) for t in dev]
    outs = [None] * 3 if capacity is None else [t.data_ptr() for t in d_out]
    rc = L.oxh_keyed_diff_device(ctx.handle, lk, case.nl, rk, case.nr, lt, rt, lv, rv, bp, flags, capacity or 0, *outs, cp,
                                 ctx.stream)
    return rc, counts.tolist(), *[t.cpu().numpy().view(a.dtype) for t, a in zip(d_out, (left, right, status))]


# ---------------------------------------------------------------- 1. sizes
SIZES = [0, 1, 63, 64, 65, 257]


@functools.lru_cache(maxsize=None)
def size_case(nl, nr):
    """Unique keys; the right side is a permutation of the left with rows dropped, added and target-changed."""
    rng = np.random.default_rng(1000 * nl + nr)
    left = rng.permutation(4 * (nl + nr) + 8)[:nl + nr].astype(np.int64)    # nl left keys, then fresh ones
    shared = min(nl, nr) - min(nl, nr) // 5                                  # about a fifth of the smaller side dropped
    right = np.concatenate([rng.permutation(left[:nl])[:shared], left[nl:nl + nr - shared]])
    right = rng.permutation(right)
    target = lambda keys: np.asarray(keys) * 7 + 3  # noqa: E731
    rt = target(right)
    changed = rng.random(nr) < 0.2
    rt[changed] += 1
    return Case(digests_of(left[:nl]), digests_of(right), digests_of(target(left[:nl])), digests_of(rt))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nl,nr", list(itertools.product(SIZES, SIZES)) + [(70001, 69997)])
def test_sizes(ctx, form, nl, nr):
    """Both sides from 0 rows to several workgroups of every launch; 70 001 rows also span several tiles of
    the scan (2 048 rows each) with a ragged tail."""
    case = size_case(nl, nr)
    want, counts, dupes = check(ctx, form, case)
    assert dupes == (0, 0) and sum(counts.values()) == nl + nr - counts[U] - counts[M]   # unique keys: a pair is one joined row
    if nl > 60 and nr > 60:
        assert counts[A] and counts[R] and counts[M] and counts[U]
    if (nl, nr) == (70001, 69997):
        check(ctx, form, case, keep=True)


# ---------------------------------------------------------------- 2. duplicated keys
GROUPS = [(1, 2), (2, 1), (2, 3), (3, 0), (0, 3), (64, 2), (1, 65), (1, 300), (300, 300)]


@functools.lru_cache(maxsize=None)
def dupes_case():
    """One group per (left, right) multiplicity among 150 unique keys per side (100 of them matched), the
    positions shuffled so that ascending row order is not insertion order; a few target values, so that the
    pairs of a group are some modified and some unchanged."""
    rng = np.random.default_rng(42)
    left, right = [], []
    for g, (a, b) in enumerate(GROUPS):
        left += [10_000 + g] * a
        right += [10_000 + g] * b
    left += list(range(150))
    right += list(range(50, 200))
    left, right = rng.permutation(left), rng.permutation(right)
    lt, rt = rng.integers(0, 3, size=left.size), rng.integers(0, 3, size=right.size)
    return Case(digests_of(left), digests_of(right), digests_of(lt), digests_of(rt))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("keep", [False, True], ids=["changed", "all"])
def test_duplicated_keys(ctx, form, keep):
    case = dupes_case()
    want, counts, dupes = check(ctx, form, case, keep)
    assert dupes == (2 + 2 + 3 + 64 + 300, 2 + 3 + 3 + 2 + 65 + 300 + 300)
    joined = sum(a * b if a and b else a + b for a, b in GROUPS) + 200
    assert sum(counts.values()) == joined and joined > case.nl + case.nr     # so the Python call had to ask twice
    if keep:
        assert len(want) == joined
    # the first call of the Python layer, by hand: nothing written, the count reported
    rc, c8, left, right, status = raw_call(ctx, form, case, int(keep), case.nl + case.nr)
    assert rc == _capi.OXH_OK and c8[0] == len(want) and c8[7] == 0 and c8[5:7] == list(dupes)
    assert (left == 0xABABABAB).all() and (right == 0xABABABAB).all() and (status == 0xAB).all()


# ---------------------------------------------------------------- 3. keys[0] nulls
@functools.lru_cache(maxsize=None)
def null_case(lbit, rbit):
    """100 left and 100 right rows with unique keys, left row i matching right row (i * 7) % 100 for i < 80.
    A null keys[0] on a matched left row (3), on a left-only row (90), on a matched right row whose left is
    valid (the partner of 5), and on both rows of a pair (8 and its partner); and the bitmaps' row 0 at
    bits lbit / rbit, with noise around them."""
    left = np.arange(100)
    right = np.empty(100, dtype=np.int64)
    right[(np.arange(80) * 7) % 100] = np.arange(80)
    free = sorted(set(range(100)) - set(((np.arange(80) * 7) % 100).tolist()))
    right[free] = 1000 + np.arange(20)
    lvalid, rvalid = np.ones(100, dtype=bool), np.ones(100, dtype=bool)
    lvalid[[3, 90, 8]] = False
    rvalid[[35, 56]] = False            # the partners of left rows 5 and 8
    target = np.arange(100) % 4         # equal on both sides of a pair: unchanged but for the nulls
    rt = np.where(right < 1000, right % 4, 0)
    return Case(digests_of(left), digests_of(right), digests_of(target), digests_of(rt), lvalid, rvalid, lbit, rbit)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("lbit,rbit", list(itertools.product([0, 3, 13], [0, 3, 13])))
def test_null_first_keys_at_bit_offsets(ctx, form, lbit, rbit):
    case = null_case(lbit, rbit)
    want, counts, dupes = check(ctx, form, case, keep=True)
    by_left = {l: (r, s) for l, r, s in want if l is not None}
    assert by_left[3] == (21, A)        # a matched left row with a null keys[0]: added
    assert by_left[90] == (None, A)     # a left-only row with one: added, not removed
    assert by_left[5] == (35, R)        # the right row's is null and the left's is not: removed
    assert by_left[8] == (56, A)        # both: the left is tested first
    assert by_left[91] == (None, R) and by_left[4] == (28, U)
    assert counts == {U: 77, A: 20 + 3, R: 19 + 1, M: 0}
    check(ctx, form, case, keep=False)


# ---------------------------------------------------------------- 4. targets
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["both", "left NULL", "right NULL", "both NULL"])
def test_target_tables_present_or_null(ctx, form, which):
    base = size_case(257, 257)
    null = null_case(3, 13)
    for c in (base, null):
        case = Case(c.lk, c.rk, None if which in ("left NULL", "both NULL") else c.lt,
                    None if which in ("right NULL", "both NULL") else c.rt, c.lvalid, c.rvalid, c.lbit, c.rbit)
        want, counts, dupes = check(ctx, form, case, keep=True)
        matched = [(l, r, s) for l, r, s in want if l is not None and r is not None]
        reach_rule_4 = [p for p in matched if p[2] in (M, U)]
        assert reach_rule_4
        if which == "both NULL":
            assert counts[M] == 0 and all(p[2] == U for p in reach_rule_4)
        elif which != "both":
            assert counts[U] == 0 and all(p[2] == M for p in reach_rule_4)   # a null column differs from every digest
        else:
            assert counts[U] and (counts[M] or c is null)


# ---------------------------------------------------------------- 5. KEEP_UNCHANGED
@pytest.mark.parametrize("form", FORMS)
def test_keep_unchanged_changes_the_pairs_not_the_counts(ctx, form):
    for case in (size_case(257, 65), dupes_case(), null_case(13, 0)):
        (with_all, counts_all, dupes_all), (changed, counts, dupes) = check(ctx, form, case, True), check(ctx, form, case, False)
        assert counts_all == counts and dupes_all == dupes
        assert changed == [p for p in with_all if p[2] != U] and len(with_all) - len(changed) == counts[U] > 0


# ---------------------------------------------------------------- 6. capacity
@pytest.mark.parametrize("form", FORMS)
def test_capacity_contract(ctx, form):
    case = dupes_case()
    want, counts, dupes = case.want(False)
    pairs = len(want)
    summary = [pairs, counts[A], counts[R], counts[M], counts[U], dupes[0], dupes[1]]
    rc, c8, *_ = raw_call(ctx, form, case, 0, None)                       # 0 with NULL arrays: counts only
    assert rc == _capi.OXH_OK and c8 == summary + [0]
    rc, c8, left, right, status = raw_call(ctx, form, case, 0, pairs - 1)  # one too few: nothing is touched
    assert rc == _capi.OXH_OK and c8 == summary + [0]
    assert (left == 0xABABABAB).all() and (right == 0xABABABAB).all() and (status == 0xAB).all()
    rc, c8, left, right, status = raw_call(ctx, form, case, 0, pairs)      # exactly enough: written
    assert rc == _capi.OXH_OK and c8 == summary + [pairs]
    assert ordered(form, triples(left, right, status), want) == want
    rc, c8, left, right, status = raw_call(ctx, form, case, 0, pairs + 3)  # more: the rest stays
    assert c8 == summary + [pairs] and (left[pairs:] == 0xABABABAB).all() and (status[pairs:] == 0xAB).all()
    assert ordered(form, triples(left[:pairs], right[:pairs], status[:pairs]), want) == want
    # an unknown flag with a live context is still OXH_ERR_INVALID
    rc, c8, *_ = raw_call(ctx, form, case, 2, pairs)
    assert rc == _capi.OXH_ERR_INVALID and c8 == [7] * 8


# ---------------------------------------------------------------- 7. digest edges
@pytest.mark.parametrize("form", FORMS)
def test_digest_edges(ctx, form):
    full = 0xFFFFFFFFFFFFFFFF
    # (0, 0) and (~0, ~0) are ordinary keys; keys equal in lo and different in hi, equal in hi and different in lo
    lk = np.array([[0, 0], [full, full], [5, 1], [5, 2], [1, 9], [2, 9], [0, full]], dtype=np.uint64)
    rk = np.array([[5, 2], [full, full], [2, 9], [0, 0], [full, 0], [5, 3], [3, 9]], dtype=np.uint64)
    t = lambda n: digests_of(np.arange(n) % 2)  # noqa: E731
    case = Case(lk, rk, t(7), t(7))
    want, counts, dupes = check(ctx, form, case, keep=True)
    assert [(l, r) for l, r, _ in want] == [(0, 3), (1, 1), (2, None), (3, 0), (4, None), (5, 2), (6, None),
                                            (None, 4), (None, 5), (None, 6)]
    assert dupes == (0, 0)
    # a left table that is all one key against a right side with no rows: every row removed, every row a dupe
    one = Case(np.tile(np.array([[7, 7]], dtype=np.uint64), (300, 1)), np.zeros((0, 2), dtype=np.uint64), t(300), None)
    want, counts, dupes = check(ctx, form, one)
    assert want == [(l, None, R) for l in range(300)] and dupes == (300, 0)
    # ... and the mirror image, and all one key on both sides (the whole cross product)
    mirror = Case(np.zeros((0, 2), dtype=np.uint64), one.lk, None, t(300))
    want, counts, dupes = check(ctx, form, mirror)
    assert want == [(None, r, A) for r in range(300)] and dupes == (0, 300)
    cross = Case(one.lk[:70], one.lk[:65], t(70), t(65))
    want, counts, dupes = check(ctx, form, cross, keep=True)
    assert len(want) == 70 * 65 and dupes == (70, 65) and counts[M] and counts[U]
    # no rows at all
    empty = Case(np.zeros((0, 2), dtype=np.uint64), np.zeros((0, 2), dtype=np.uint64))
    assert check(ctx, form, empty)[0] == []


# ---------------------------------------------------------------- 8. end to end
def test_diff_dfs_over_two_frames(ctx, oracle_lib):
    n = 500
    rng = np.random.default_rng(9)
    ids = rng.permutation(2 * n)[:n].astype(np.int64)
    id_valid = rng.random(n) > 0.03
    names = ["k%d" % (i % 211) for i in range(n)]
    score = rng.standard_normal(n)
    note = [None if i % 17 == 0 else "n%d" % (i % 5) for i in range(n)]
    left = {"id": column(ids, validity=id_valid), "name": column(names), "score": column(score), "note": column(note),
            "old": column(np.arange(n, dtype=np.int32))}
    keep = rng.permutation(n)[: n - 40]                      # 40 rows dropped, the rest shuffled
    r_ids, r_valid = ids[keep].copy(), id_valid[keep].copy()
    r_names = [names[i] for i in keep]
    r_score, r_note = score[keep].copy(), [note[i] for i in keep]
    r_score[rng.random(keep.size) < 0.1] += 1.0             # targets changed
    r_note[3], r_note[4] = "changed", None
    r_valid[[10, 11]] = False                               # nulls the left side does not have: other key digests, no match
    extra = 30                                               # rows added
    right = {"id": column(np.concatenate([r_ids, 5000 + np.arange(extra)]), validity=np.concatenate([r_valid, np.ones(extra, bool)])),
             "name": column(r_names + ["new%d" % i for i in range(extra)]),
             "score": column(np.concatenate([r_score, np.zeros(extra)])), "note": column(r_note + ["x"] * extra),
             "new": column(np.ones(keep.size + extra, dtype=bool))}

    def restated(keys, targets, key0):
        on = lambda f, names: _rowhash.row_hashes([c for k, c in f.items() if k in names], oracle_lib)  # noqa: E731
        valid = lambda c: None if c.validity is None else _rowhash.bits(c.validity, c.validity_bit, c.nrows).tolist()  # noqa: E731
        lt = on(left, targets) if any(t in left for t in targets) else None
        rt = on(right, targets) if any(t in right for t in targets) else None
        return _keyeddiff.keyed_diff(rows_of(on(left, keys)), rows_of(on(right, keys)), rows_of(lt), rows_of(rt),
                                     valid(left[key0]), valid(right[key0]))

    for keys, targets, want_keys, want_targets in (
            (["id", "name"], ["score", "note"], ["id", "name"], ["score", "note"]),
            (["name", "id"], [], ["id", "name"], ["score", "note"]),                    # targets default; keys[0] = name: no nulls
            ([], [], ["id", "name", "score", "note"], ["new", "old"])):
        pairs, counts, dupes = restated(want_keys, want_targets, keys[0] if keys else "id")
        d = tabular.diff_dfs(left, right, keys=keys, targets=targets, ctx=ctx)
        got = [(None if l < 0 else l, None if r < 0 else r, s)
               for l, r, s in zip(d.left_rows.tolist(), d.right_rows.tolist(), d.status.tolist())]
        assert got == pairs
        assert (d.added, d.removed, d.modified, d.unchanged) == (counts[A], counts[R], counts[M], counts[U])
        assert (d.dupes_left, d.dupes_right) == dupes
        assert d.added and d.removed and d.modified
    # "id" has nulls on the left and is keys[0] in the first case: some matched pairs are `added`
    pairs, counts, _ = restated(["id", "name"], ["score", "note"], "id")
    assert any(s == A and l is not None and r is not None for l, r, s in pairs)


# ---------------------------------------------------------------- 9. repeatability
def test_the_same_call_twice_and_the_contexts_own_index(ctx):
    from oxen_amd.dedup import DedupIndex

    case = dupes_case()
    mine = digests_of(50_000 + np.arange(1000) % 600)
    with DedupIndex(ctx) as index:
        first, _ = index.insert(mine)
        before = index.counts()
        a = raw_call(ctx, "host", case, 1, 200_000)
        b = raw_call(ctx, "host", case, 1, 200_000)
        assert a[0] == _capi.OXH_OK and a[1] == b[1] and a[1][7] == a[1][0] > 0
        for x, y in zip(a[2:], b[2:]):
            assert np.array_equal(x, y)                    # the host form's order is fixed
        for form in FORMS:
            check(ctx, form, case)
        # the context's own index is what it was: nothing of the diff's rows is in it
        assert index.counts() == before
        assert np.array_equal(index.query(mine), first)
        absent = index.query(np.concatenate([case.lk[:50], case.rk[:50]]))
        assert (absent == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
