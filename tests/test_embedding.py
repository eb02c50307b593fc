"""The embedding query on the GPU (oxh_embedding_*, oxen_amd/csrc/embedding.hip; oxen_amd.tabular): the mean of
the selected vectors, the cosine similarity of every row with its order key and permutation, and the take of a
page's vectors, both forms. The outputs are filled with sentinels first and the WHOLE arrays are compared with
the restatement of tests/_embedding.py: tails, bits past nrows and untouched outputs included.

Exact tests use integer-valued floats in [-8, 8]: with dim <= 4097 every partial sum is an integer below 2^24 in
any order, so dot, nx and nq are exact and sim must equal numpy's float32 dot / sqrt(nx * nq) bit for bit; the
same inputs make the mean exact. The thresholds between the kernel's shapes and the sizes of its grids are read
from the sources."""
import functools
import os
import re

import numpy as np
import pytest

import _embedding as E
import _filterrows
import _take
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, Embedding, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
LAYOUTS = [E.FIXED, E.LIST32, E.LIST64]
SENTINEL = 0x5A5A5A5A
SENTINEL_F = np.uint32(SENTINEL).view(np.float32)
UNTOUCHED_BYTE = 0xA5
INVALID, OK = _capi.OXH_ERR_INVALID, _capi.OXH_OK
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCE = open(os.path.join(CSRC, "embedding.hip")).read()
HOST_SOURCE = open(os.path.join(CSRC, "embedding_host.hpp")).read()
QUAD_MAX, SUBWAVE_MAX = (int(x) for x in re.search(r"constexpr uint32_t kEmbQuadDimMax = (\d+), kEmbSubwaveDimMax = (\d+);", SOURCE).groups())
CAP = int(re.search(r"constexpr uint32_t kEmbGridCap = (\d+);", SOURCE).group(1))
MEAN_CHUNK, MEAN_GROUPS = (int(x) for x in re.search(r"constexpr uint32_t kMeanChunk = (\d+), kMeanMaxGroups = (\d+);", HOST_SOURCE).groups())
assert re.search(r"constexpr int TASK = LPR == 64 \? 8 : 64;", SOURCE) and CAP == 2048
ROUND_SUBWAVE = CAP * 4 * 64          # rows of one round of the capped grid with several rows per wave: 4 waves x 64 rows
ROUND_WAVE = CAP * 4 * 8              # and with a wave per row: tasks of 8 rows
MEAN_ROUND = MEAN_CHUNK * MEAN_GROUPS  # idx entries of one round of the mean's grid
DIMS = sorted({1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 768, 1025, 4097,
               QUAD_MAX - 1, QUAD_MAX, QUAD_MAX + 1, SUBWAVE_MAX - 1, SUBWAVE_MAX, SUBWAVE_MAX + 1})


# ---------------------------------------------------------------- helpers
def at_phase(values, phase):
    """A float32 copy of `values` whose address is 4 * phase bytes past a 16-byte boundary."""
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    raw = np.zeros(4 * values.size + 32, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + 4 * phase
    view = raw[start:start + 4 * values.size].view(np.float32)
    view[:] = values
    assert view.size == 0 or view.ctypes.data % 16 == 4 * phase
    return view


def build(x, valid=None, layout=E.FIXED, phase=0, vbit=0, first=0, lengths=None):
    """An Embedding over the rows of x (n, dim): `first` elements in front of a list column's first row, the values
    at `phase`, the validity's row 0 at bit `vbit` (None: no validity). lengths: a list column's row lengths
    where they are not dim (the row's elements are then the first of x's row, or those and zeros)."""
    n, d = x.shape
    validity = None if valid is None else E.packed_at(valid, vbit)
    if layout == E.FIXED:
        return Embedding(layout, d, n, at_phase(x, phase), None, validity, vbit if valid is not None else 0)
    lens = np.full(n, d, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    pieces = [np.full(first, 77, dtype=np.float32)]
    for r in range(n):
        row = np.zeros(lens[r], dtype=np.float32)
        row[:min(d, lens[r])] = x[r, :min(d, lens[r])]
        pieces.append(row)
    offsets = (first + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32 if layout == E.LIST32 else np.int64)
    return Embedding(layout, d, n, at_phase(np.concatenate(pieces), phase), offsets, validity, vbit if valid is not None else 0)


def device_floats(a):
    """A float32 device tensor with the bytes of `a` at a's own phase within 16 bytes."""
    import torch

    a = np.ascontiguousarray(a)
    phase = a.ctypes.data % 16 if a.size else 0
    t = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device="cuda:0")
    start = (-t.data_ptr()) % 16 + phase
    piece = t[start:start + a.nbytes]
    piece.copy_(torch.from_numpy(a.view(np.uint8).copy()))
    return piece.view(torch.float32)


def tensor(a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda:0")


def device_embedding(emb):
    return emb._replace(values=device_floats(emb.values), offsets=tensor(emb.offsets), validity=tensor(emb.validity))


def host_ptr(keep):
    def ptr(a):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(a))
        return keep[-1].ctypes.data if keep[-1].size else None
    return ptr


dev_ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731


class Got:
    def __init__(self, rc, stats, **arrays):
        self.rc, self.stats = rc, stats
        self.__dict__.update(arrays)


def similarity_call(ctx, form, emb, q, validity=True, key=True, perm=True):
    """The ABI itself, the outputs filled with sentinels first: the status, stats4 (7s where the call wrote none)
    and the whole sim, validity, order_key and perm arrays."""
    import torch

    n, nb = emb.nrows, -(-emb.nrows // 8)
    stats = np.full(4, 7, dtype=np.uint64)
    L, q = _capi.lib(), np.ascontiguousarray(q, dtype=np.float32)
    if form == "host":
        keep = []
        ptr = host_ptr(keep)
        sim, bitmap = np.full(n, SENTINEL_F, np.float32), np.full(nb, UNTOUCHED_BYTE, np.uint8)
        keys, order = np.full(n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32)
        rc = L.oxh_embedding_similarity_host(ctx.handle, *tabular._embedding_args(emb, ptr), ptr(q), ptr(sim), ptr(bitmap) if validity else None,
                                             ptr(keys) if key else None, ptr(order) if perm else None, stats.ctypes.data_as(_capi._u64p))
        return Got(rc, tuple(stats.tolist()), sim=sim, validity=bitmap, key=keys, perm=order)
    dev = device_embedding(emb)
    sim = torch.full((n,), float(SENTINEL_F), dtype=torch.float32, device="cuda:0")
    bitmap = torch.full((nb,), UNTOUCHED_BYTE, dtype=torch.uint8, device="cuda:0")
    keys = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
    order = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
    dq = device_floats(q)
    torch.cuda.synchronize()
    rc = L.oxh_embedding_similarity_device(ctx.handle, *tabular._embedding_args(dev, dev_ptr), dev_ptr(dq), dev_ptr(sim),
                                           dev_ptr(bitmap) if validity else None, dev_ptr(keys) if key else None,
                                           dev_ptr(order) if perm else None, stats.ctypes.data_as(_capi._u64p), ctx.stream)
    torch.cuda.synchronize()
    return Got(rc, tuple(stats.tolist()), sim=sim.cpu().numpy(), validity=bitmap.cpu().numpy(), key=keys.cpu().numpy().view(np.uint32),
               perm=order.cpu().numpy().view(np.uint32))


def mean_call(ctx, form, emb, idx):
    import torch

    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    stats = np.full(4, 7, dtype=np.uint64)
    L = _capi.lib()
    if form == "host":
        keep = []
        ptr = host_ptr(keep)
        out = np.full(emb.dim, SENTINEL_F, np.float32)
        rc = L.oxh_embedding_mean_host(ctx.handle, *tabular._embedding_args(emb, ptr), ptr(idx), idx.size, ptr(out), stats.ctypes.data_as(_capi._u64p))
        return Got(rc, tuple(stats.tolist()), out=out)
    dev, didx = device_embedding(emb), tensor(idx)
    out = torch.full((emb.dim,), float(SENTINEL_F), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = L.oxh_embedding_mean_device(ctx.handle, *tabular._embedding_args(dev, dev_ptr), dev_ptr(didx), idx.size, dev_ptr(out),
                                     stats.ctypes.data_as(_capi._u64p), ctx.stream)
    torch.cuda.synchronize()
    return Got(rc, tuple(stats.tolist()), out=out.cpu().numpy())


def take_call(ctx, form, emb, idx):
    import torch

    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    n, nb = idx.size, -(-idx.size // 8)
    stats = np.full(4, 7, dtype=np.uint64)
    L = _capi.lib()
    if form == "host":
        keep = []
        ptr = host_ptr(keep)
        out, bitmap = np.full(n * emb.dim, SENTINEL_F, np.float32), np.full(nb, UNTOUCHED_BYTE, np.uint8)
        rc = L.oxh_embedding_take_host(ctx.handle, *tabular._embedding_args(emb, ptr), ptr(idx), n, ptr(out), ptr(bitmap),
                                       stats.ctypes.data_as(_capi._u64p))
        return Got(rc, tuple(stats.tolist()), out=out, validity=bitmap)
    dev, didx = device_embedding(emb), tensor(idx)
    out = torch.full((n * emb.dim,), float(SENTINEL_F), dtype=torch.float32, device="cuda:0")
    bitmap = torch.full((nb,), UNTOUCHED_BYTE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = L.oxh_embedding_take_device(ctx.handle, *tabular._embedding_args(dev, dev_ptr), dev_ptr(didx), n, dev_ptr(out), dev_ptr(bitmap),
                                     stats.ctypes.data_as(_capi._u64p), ctx.stream)
    torch.cuda.synchronize()
    return Got(rc, tuple(stats.tolist()), out=out.cpu().numpy(), validity=bitmap.cpu().numpy())


def same_floats(got, want, who):
    """Bit for bit, but a NaN equals any NaN (the sign and payload of an invalid operation's NaN are the machine's)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (who, got.shape, want.shape)
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if differ.any():
        at = int(np.nonzero(differ)[0][0])
        raise AssertionError((who, "first difference at", at, got[at:at + 4].tolist(), want[at:at + 4].tolist()))


def same_array(got, want, who):
    assert got.shape == want.shape, (who, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError((who, "first difference at", at, got[at:at + 4].tolist(), want[at:at + 4].tolist()))


def same_similarity(got, want, who, rc=OK, untouched=False, validity=True, key=True, perm=True):
    """The whole outputs against the restatement's. untouched: the call must have written nothing but stats4."""
    assert got.rc == rc, (who, got.rc, _capi.lib().oxh_last_error())
    assert got.stats == want.stats, (who, got.stats, want.stats)
    n = want.sim.size
    same_floats(got.sim, np.full(n, SENTINEL_F, np.float32) if untouched else want.sim, (who, "sim"))
    same_array(got.validity, want.validity if validity and not untouched else np.full(-(-n // 8), UNTOUCHED_BYTE, np.uint8), (who, "validity"))
    same_array(got.key, want.key if key and not untouched else np.full(n, SENTINEL, np.uint32), (who, "key"))
    same_array(got.perm, want.perm if perm and not untouched else np.full(n, SENTINEL, np.uint32), (who, "perm"))
    if not untouched and key:
        # exact whatever the rounding: the key is the key function of the RETURNED sim, perm the stable sort of the RETURNED key
        valid = E.bits(got.validity, 0, n) if validity else np.ones(n, bool)
        expect = np.array([E.order_key(int(b)) if ok else E.NULL_KEY for b, ok in zip(got.sim.view(np.uint32).tolist(), valid.tolist())], np.uint32)
        same_array(got.key, expect, (who, "key of the returned sim"))
        if perm:
            same_array(got.perm, E.stable_order(got.key), (who, "perm of the returned key"))


def exact_want(x, valid, q, not_read=()):
    """The restatement for integer-valued rows x (n, dim) in any layout: `not_read` rows rank as nulls and count
    as rows of another length."""
    ok = np.ones(x.shape[0], bool) if valid is None else np.asarray(valid, bool).copy()
    wrong = [r for r in not_read if ok[r]]
    ok[wrong] = False
    want = E.similarity_exact(tabular.embedding(x, ok), q)
    nulls = x.shape[0] - int(ok.sum()) - len(wrong)
    want.stats = (int(ok.sum()), nulls, len(wrong), min(wrong) if wrong else x.shape[0])
    return want


def integers(rng, n, d):
    return rng.integers(-8, 9, size=(n, d)).astype(np.float32)


def some_valid(rng, n):
    return rng.random(n) > 0.25


# ---------------------------------------------------------------- 1. similarity, exact
@pytest.mark.parametrize("dim", DIMS)
def test_similarity_is_exact_at_every_dim(ctx, dim):
    """Every dim around the kernel's three shapes and their 16-byte pieces, each with another layout, phase of the
    values within 16 bytes, first bit of the validity and first offset; both forms."""
    k = DIMS.index(dim)
    rng = np.random.default_rng(100 + dim)
    n = (65, 64, 63, 130)[k % 4]
    x, q, valid = integers(rng, n, dim), integers(rng, 1, dim)[0], some_valid(rng, n)
    for j, layout in enumerate(LAYOUTS):
        emb = build(x, valid, layout, phase=(k + j) % 4, vbit=(0, 3, 7)[(k + j) % 3], first=(0, 5, 2)[j])
        want = exact_want(x, valid, q)
        for form in FORMS:
            same_similarity(similarity_call(ctx, form, emb, q), want, (form, dim, layout))


@pytest.mark.parametrize("dim", [1, 4, 5, 17, 257])
def test_similarity_rows_phases_and_validity_bits(ctx, dim):
    """Rows 1, 63, 64, 65 x the three layouts x the values at every 4-byte phase of 16 x validity from bits 0, 3, 7
    (and none); list columns whose first offset is not 0."""
    rng = np.random.default_rng(200 + dim)
    q = integers(rng, 1, dim)[0]
    for n in (1, 63, 64, 65):
        x = integers(rng, n, dim)
        for layout in LAYOUTS:
            for phase in range(4):
                vbit = (0, 3, 7, None)[(phase + n) % 4]
                valid = None if vbit is None else some_valid(rng, n)
                emb = build(x, valid, layout, phase, vbit or 0, first=(0, 3)[phase % 2] + phase)
                want = exact_want(x, valid, q)
                form = FORMS[(phase + LAYOUTS.index(layout)) % 2]
                same_similarity(similarity_call(ctx, form, emb, q, validity=valid is not None), want, (form, dim, n, layout, phase, vbit),
                                validity=valid is not None)
    # sim alone, and sim with its keys: what is not asked for is not written
    x, valid = integers(rng, 65, dim), some_valid(rng, 65)
    for form in FORMS:
        emb, want = build(x, valid, E.LIST32, 1, 3, 4), exact_want(x, valid, q)
        same_similarity(similarity_call(ctx, form, emb, q, key=False, perm=False), want, (form, "sim alone"), key=False, perm=False)
        same_similarity(similarity_call(ctx, form, emb, q, perm=False), want, (form, "no perm"), perm=False)


@pytest.mark.parametrize("dim,n", [(1, ROUND_SUBWAVE - 1), (1, ROUND_SUBWAVE), (1, ROUND_SUBWAVE + 1), (1, 2 * ROUND_SUBWAVE + 37),
                                   (4, ROUND_SUBWAVE - 1), (4, ROUND_SUBWAVE + 1), (4, 2 * ROUND_SUBWAVE + 37),
                                   (SUBWAVE_MAX + 1, ROUND_WAVE + 1)])
def test_similarity_past_the_capped_grid(ctx, dim, n):
    """One full round of the capped grid +- 1 and two rounds plus a ragged tail: every wave loops."""
    rng = np.random.default_rng(n + dim)
    x, q = integers(rng, n, dim), integers(rng, 1, dim)[0]
    q[0] = 3.0   # not a zero query
    valid = some_valid(rng, n)
    emb, want = build(x, valid, E.FIXED, phase=1, vbit=3), exact_want(x, valid, q)
    same_similarity(similarity_call(ctx, "device", emb, q), want, ("device", dim, n))
    if n == 2 * ROUND_SUBWAVE + 37:
        same_similarity(similarity_call(ctx, "host", emb, q), want, ("host", dim, n))


# ---------------------------------------------------------------- 2. the order
@pytest.mark.parametrize("form", FORMS)
def test_order_ties_nans_and_nulls(ctx, form):
    dim = 4
    q = np.array([1, 0, 0, 0], np.float32)
    # many tied similarities: multiples of one vector tie at +1 / -1, orthogonal rows at 0 (+0.0 and -0.0 tie too)
    base = np.array([[2, 0, 0, 0], [0, 3, 0, 0], [-1, 0, 0, 0], [5, 0, 0, 0], [0, 0, -2, 0], [-7, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]], np.float32)
    x = np.tile(base, (20, 1))
    valid = np.ones(x.shape[0], bool)
    valid[[3, 11, 40]] = False
    want = exact_want(x, valid, q)
    got = similarity_call(ctx, form, build(x, valid, E.LIST64, 2, 7, 1), q)
    same_similarity(got, want, (form, "ties"))
    n = x.shape[0]
    order = got.perm.tolist()
    zero_rows = [r for r in range(n) if r % 8 == 7 and valid[r]]
    assert order[:len(zero_rows)] == zero_rows                      # a zero row is NaN: first, in input order
    ones = [r for r in range(n) if r % 8 in (0, 3) and valid[r]]
    assert order[len(zero_rows):len(zero_rows) + len(ones)] == ones   # ties come in input order
    assert order[-3:] == [3, 11, 40]                                  # nulls last
    assert np.isnan(got.sim[zero_rows]).all() and (got.sim[ones] == 1).all()
    # all rows null; no validity at all (sim_validity NULL, and given: all ones)
    nothing = np.zeros(n, bool)
    same_similarity(similarity_call(ctx, form, build(x, nothing, E.FIXED, 3, 3), q), exact_want(x, nothing, q), (form, "all null"))
    want = exact_want(x, None, q)
    same_similarity(similarity_call(ctx, form, build(x), q, validity=False), want, (form, "no validity"), validity=False)
    same_similarity(similarity_call(ctx, form, build(x), q), want, (form, "no validity, bitmap given"))
    # NaN and inf elements propagate as IEEE says; the order is checked on the returned arrays
    y = integers(np.random.default_rng(9), 70, 5)
    y[3, 2], y[10, 0], y[20, 4], y[30, 1] = np.nan, np.inf, -np.inf, np.inf
    y[30, 3] = -np.inf
    q5 = np.array([1, 2, 0, -1, 3], np.float32)
    got = similarity_call(ctx, form, build(y, None, E.LIST32, 1), q5)
    assert got.rc == OK and got.stats == (70, 0, 0, 70)
    assert np.isnan(got.sim[[3, 10, 20, 30]]).all()       # inf / sqrt(inf) and inf - inf are NaN
    clean = [r for r in range(70) if r not in (3, 10, 20, 30)]
    same_floats(got.sim[clean], exact_want(y[clean], None, q5).sim, (form, "rows beside the NaNs"))
    expect = np.array([E.order_key(int(b)) for b in got.sim.view(np.uint32).tolist()], np.uint32)
    same_array(got.key, expect, (form, "keys"))
    same_array(got.perm, E.stable_order(got.key), (form, "perm"))
    assert got.perm[:4].tolist() == [3, 10, 20, 30]
    # a zero query: every similarity is NaN, the order is the input order
    got = similarity_call(ctx, form, build(y[clean]), np.zeros(5, np.float32))
    assert got.rc == OK and np.isnan(got.sim).all() and got.perm.tolist() == list(range(len(clean)))


# ---------------------------------------------------------------- 3. the mean
def exact_mean(x, valid, idx):
    """Integer sums divided by a count: exact whatever the order."""
    used = [int(r) for r in idx if valid is None or valid[int(r)]]
    stats = (len(used), len(idx) - len(used), 0, x.shape[0])
    if not used:
        return None, stats
    return (x[used].astype(np.float64).sum(axis=0).astype(np.float32) / np.float32(len(used))).astype(np.float32), stats


def same_mean(got, want, stats, who, rc=OK):
    assert got.rc == rc, (who, got.rc, _capi.lib().oxh_last_error())
    assert got.stats == stats, (who, got.stats, stats)
    same_floats(got.out, np.full(got.out.size, SENTINEL_F, np.float32) if want is None else want, who)   # no row used: untouched


@pytest.mark.parametrize("dim", [1, 3, 8, 255, 256, 257, 768])
def test_mean_is_exact(ctx, dim):
    rng = np.random.default_rng(300 + dim)
    n = 600
    x, valid = integers(rng, n, dim), some_valid(rng, n)
    k = [1, 3, 8, 255, 256, 257, 768].index(dim)
    layout, phase, vbit = LAYOUTS[k % 3], k % 4, (0, 3, 7)[k % 3]
    emb = build(x, valid, layout, phase, vbit, first=k)
    for nidx in (1, 2, 255, 256, 257):
        idx = np.sort(rng.choice(n, nidx, replace=False)).astype(np.uint32)
        want, stats = exact_mean(x, valid, idx)
        for form in FORMS:
            same_mean(mean_call(ctx, form, emb, idx), want, stats, (form, dim, nidx))
    everything = np.arange(n, dtype=np.uint32)                        # idx with all rows: nulls interleaved
    only_nulls = np.nonzero(~valid)[0].astype(np.uint32)              # idx with only null rows: zero used
    no_validity = build(x, None, layout, phase)
    for form in FORMS:
        same_mean(mean_call(ctx, form, emb, everything), *exact_mean(x, valid, everything), (form, dim, "all rows"))
        same_mean(mean_call(ctx, form, emb, only_nulls), *exact_mean(x, valid, only_nulls), (form, dim, "only nulls"))
        same_mean(mean_call(ctx, form, emb, np.zeros(0, np.uint32)), None, (0, 0, 0, n), (form, dim, "no index"))
        same_mean(mean_call(ctx, form, no_validity, everything), *exact_mean(x, None, everything), (form, dim, "no validity"))


@pytest.mark.parametrize("nidx", [MEAN_ROUND - 1, MEAN_ROUND, MEAN_ROUND + 1])
def test_mean_past_one_round_of_its_grid(ctx, nidx):
    rng = np.random.default_rng(nidx)
    n, dim = MEAN_ROUND + 300, 3
    x, valid = integers(rng, n, dim), some_valid(rng, n)
    idx = np.sort(rng.choice(n, nidx, replace=False)).astype(np.uint32)
    emb = build(x, valid, E.FIXED, 1, 3)
    want, stats = exact_mean(x, valid, idx)
    for form in FORMS:
        same_mean(mean_call(ctx, form, emb, idx), want, stats, (form, nidx))


def test_mean_is_identical_from_run_to_run_and_between_the_forms(ctx):
    """Random normal data, where the order of the additions shows: the partition is fixed, so the bits are."""
    rng = np.random.default_rng(7)
    for n, dim, nidx in ((5000, 768, 3000), (MEAN_ROUND + 500, 5, MEAN_ROUND + 100), (300, 64, 1)):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        valid = some_valid(rng, n)
        idx = np.sort(rng.choice(n, nidx, replace=False)).astype(np.uint32)
        emb = build(x, valid, E.LIST32, 3, 3, 2)
        runs = [mean_call(ctx, form, emb, idx) for form in ("device", "device", "host", "host")]
        for other in runs[1:]:
            assert other.rc == OK and other.stats == runs[0].stats
            same_array(other.out.view(np.uint32), runs[0].out.view(np.uint32), (n, dim, nidx))
        # and within n * 2^-24 * sum |x| per element of the float64 mean
        used = [int(r) for r in idx if valid[int(r)]]
        if used:
            exact = x[used].astype(np.float64).mean(axis=0)
            # the sum: gamma_n sum |x| <= 1.01 n 2^-24 sum |x| at these n; divided by n; then the division's own rounding
            bound = 1.01 * 2.0 ** -24 * np.abs(x[used].astype(np.float64)).sum(axis=0) + 2.0 ** -24 * np.abs(exact)
            assert (np.abs(runs[0].out.astype(np.float64) - exact) <= bound).all(), (n, dim, nidx)


# ---------------------------------------------------------------- 4. the take
@pytest.mark.parametrize("layout", LAYOUTS)
def test_take_gathers_a_page(ctx, layout):
    rng = np.random.default_rng(400 + layout)
    for dim, nout in ((1, 1), (3, 63), (8, 64), (17, 65), (768, 10), (5, 300)):
        n = 200
        x, valid = integers(rng, n, dim), some_valid(rng, n)
        emb = build(x, valid, layout, phase=dim % 4, vbit=(0, 3, 7)[dim % 3], first=dim % 5)
        idx = rng.integers(0, n, nout).astype(np.uint32)
        idx[rng.random(nout) < 0.2] = E.TAKE_NULL
        values, bitmap, stats = E.take(emb, idx)
        for form in FORMS:
            got = take_call(ctx, form, emb, idx)
            assert got.rc == OK and got.stats == stats, (form, dim, nout, got.rc, got.stats, stats)
            same_floats(got.out, values, (form, dim, nout))
            same_array(got.validity, bitmap, (form, dim, nout, "validity"))
    absent = np.full(9, E.TAKE_NULL, np.uint32)
    for form in FORMS:
        got = take_call(ctx, form, emb, absent)
        assert got.rc == OK and got.stats == (0, 9, 0, n) and not got.out.any() and got.validity.tolist() == [0, 0]


# ---------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("layout", [E.LIST32, E.LIST64])
def test_rows_of_another_length_are_refused_and_counted(ctx, layout):
    """A valid list row of length dim +- 1, at the first, the last and a middle row: OXH_ERR_INVALID after the
    kernels have finished, with the stats right. The device form has written its outputs (the row ranks as a
    null); the host form leaves the caller's arrays untouched. Every span lies inside the values: these are
    refusals, not faults."""
    rng = np.random.default_rng(500 + layout)
    n, dim = 70, 5
    x, q = integers(rng, n, dim), np.array([1, -1, 2, 0, 3], np.float32)
    valid = np.ones(n, bool)
    valid[[7, 8]] = False
    for where in (0, n - 1, 33):
        for delta in (-1, 1):
            lengths = np.full(n, dim)
            lengths[where] = dim + delta
            lengths[7] = 2          # a null row's span is not looked at
            emb = build(x, valid, layout, phase=where % 4, vbit=3, first=3, lengths=lengths)
            want = exact_want(x, valid, q, not_read=[where])
            assert want.stats == (n - 3, 2, 1, where)
            for form in FORMS:
                got = similarity_call(ctx, form, emb, q)
                same_similarity(got, want, (form, where, delta), rc=INVALID, untouched=form == "host")
                assert b"not of length dim" in _capi.lib().oxh_last_error()
                idx = np.array(sorted({0, 5, 7, where, n - 1}), np.uint32)
                used = [r for r in idx.tolist() if valid[r] and r != where]
                got = mean_call(ctx, form, emb, idx)
                assert got.rc == INVALID and got.stats == (len(used), 1, 1, where), (form, where, delta, got.stats)
                if form == "device":   # the mean of the rows that were read
                    same_floats(got.out, exact_mean(x, None, used)[0], (form, where, delta))
                else:
                    same_floats(got.out, np.full(dim, SENTINEL_F, np.float32), (form, where, delta, "untouched"))
                got = take_call(ctx, form, emb, np.array([where, 1, E.TAKE_NULL], np.uint32))
                assert got.rc == INVALID and got.stats == (1, 1, 1, where), (form, where, delta, got.stats)
                if form == "device":
                    same_floats(got.out, np.concatenate([np.zeros(dim, np.float32), x[1], np.zeros(dim, np.float32)]), (form, "take"))
                    assert got.validity.tolist() == [0b010]
    # two such rows: the stats name the smaller
    lengths = np.full(n, dim)
    lengths[[60, 20]] = (dim + 1, dim - 1)
    got = similarity_call(ctx, "device", build(x, valid, layout, lengths=lengths), q)
    assert got.rc == INVALID and got.stats == (n - 4, 2, 2, 20)


def test_decreasing_offsets_and_indices_past_the_rows_are_refused(ctx):
    rng = np.random.default_rng(6)
    n, dim = 40, 3
    x, q = integers(rng, n, dim), np.array([1, 2, 3], np.float32)
    emb = build(x, None, E.LIST32, first=6)
    down = emb.offsets.copy()
    down[11] -= 5                       # rows 10 and 11: offsets decrease between them; every offset stays inside values
    bad = emb._replace(offsets=down)
    for form in FORMS:
        got = similarity_call(ctx, form, bad, q)
        assert got.rc == INVALID and b"decrease" in _capi.lib().oxh_last_error(), (form, got.rc)
        if form == "host":              # checked before anything is copied: nothing is written, stats4 included
            assert got.stats == (7, 7, 7, 7) and (got.key == SENTINEL).all()
        else:                           # row 10's pair decreases (not read); row 11 is of another length
            assert got.stats == (n - 2, 0, 1, 11) and got.key[10] == E.NULL_KEY and got.key[11] == E.NULL_KEY
            keep = [r for r in range(n) if r not in (10, 11)]
            same_floats(got.sim[keep], exact_want(x[keep], None, q).sim, "rows beside the bad pair")
        # an idx entry equal to nrows: the mean and the take refuse it and read nothing through it
        for call, idx in ((mean_call, [0, 3, n]), (take_call, [3, n, 0])):
            got = call(ctx, form, emb, np.array(idx, np.uint32))
            assert got.rc == INVALID and (b"not a row" in _capi.lib().oxh_last_error() or b"nor a row" in _capi.lib().oxh_last_error()), (form, idx)
    got = mean_call(ctx, "device", emb, np.array([0, 3, n], np.uint32))
    assert got.stats == (2, 0, 0, n)
    same_floats(got.out, exact_mean(x, None, [0, 3])[0], "the rows that are rows")


# ---------------------------------------------------------------- 6. tolerance
@pytest.mark.parametrize("dim", [3, 64, 768])
def test_similarity_of_random_vectors_within_the_derived_bound(ctx, dim):
    """|sim - exact| <= (2 dim + 8) 2^-24: gamma_dim on the dot product (sum |x q| <= |x| |q|), gamma_dim on the
    norms, four single roundings -- whatever the order of the sums."""
    rng = np.random.default_rng(600 + dim)
    n = 257
    x, q = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
    xd, qd = x.astype(np.float64), q.astype(np.float64)
    exact = (xd @ qd) / np.sqrt((xd * xd).sum(axis=1) * (qd * qd).sum())
    bound = (2 * dim + 8) * 2.0 ** -24
    for j, form in enumerate(FORMS):
        got = similarity_call(ctx, form, build(x, None, LAYOUTS[(dim + j) % 3], phase=1 + j, first=3), q)
        assert got.rc == OK and got.stats == (n, 0, 0, n)
        worst = float(np.abs(got.sim.astype(np.float64) - exact).max())
        print(f"dim {dim} {form}: worst |sim - exact| = {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, (form, dim, worst, bound)
        same_array(got.perm, E.stable_order(got.key), (form, dim, "perm"))


# ---------------------------------------------------------------- 7. the chain
@functools.lru_cache(maxsize=None)
def chain_frame():
    """1 000 rows: an Int64 id, a string label, a nullable embedding of 8 integer-valued floats. Five rows are
    labelled `pick`, one of them without an embedding: the mean of the other four is exact (quarters), and so is
    every similarity with it."""
    rng = np.random.default_rng(77)
    n = 1000
    ids = np.arange(n, dtype=np.int64)
    labels = [("dog", "cat", "bird")[i % 3] for i in range(n)]
    for i in (42, 99, 500, 640, 901):
        labels[i] = "pick"
    x = integers(rng, n, 8)
    x[100:110] = x[42]                   # tied rows
    x[300] = 0                           # a zero row: NaN, first
    valid = rng.random(n) > 0.1
    valid[[42, 99, 640, 901, 300]] = True
    valid[100:110] = True
    valid[500] = False
    frame = {"id": column(ids), "label": column(labels)}
    return frame, x, valid


def chain_want(where, page_size, page_num):
    frame, x, valid = chain_frame()
    cols = list(frame.values())
    terms, logical = tabular.filter_terms(frame, where)
    selected = _filterrows.filter_rows(cols, terms, logical, [_filterrows.SIGNED] * 2)
    emb = tabular.embedding(x, valid)
    mean, _ = E.mean(emb, selected.idx)
    ranked = E.similarity_exact(emb, mean)
    first, count = E.page_rows(1000, page_size, page_num)
    rows = ranked.perm[first:first + count]
    sim = Column(4, 1000, ranked.sim, None, ranked.validity, 0, 0)
    return _take.take(cols + [sim], rows), E.take(emb, rows), rows


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("where", ["id == 42", "label == pick"])
def test_sort_by_similarity_pages(ctx, form, where):
    """`sort_by_similarity` against the restatement composed from _filterrows, _embedding and _take: pages 0, 1, the
    last partial page and a page past the end; the page round-trips through pyarrow."""
    import torch

    pa = pytest.importorskip("pyarrow")
    frame, x, valid = chain_frame()
    emb = build(x, valid, E.LIST32 if form == "host" else E.FIXED, phase=1, vbit=3, first=2 if form == "host" else 0)
    if form == "device":
        dframe = {k: Column(c.kind, c.nrows, tensor(c.values), tensor(c.offsets), tensor(c.validity), 0, 0) for k, c in frame.items()}
        demb = device_embedding(emb)
    for page_size, page_num in ((100, 0), (100, 1), (64, 16), (300, 4), (100, 11), (100, 12)):
        want_cols, (want_values, want_bitmap, _), rows = chain_want(where, page_size, page_num)
        if form == "host":
            page = tabular.sort_by_similarity(frame, emb, where, page_size, page_num, ctx=ctx)
        else:
            page = tabular.sort_by_similarity_device(dframe, demb, where, page_size, page_num, stream=ctx.stream, ctx=ctx)
            torch.cuda.synchronize()
            host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
            page = {k: (v._replace(values=host(v.values), offsets=host(v.offsets), validity=host(v.validity))) for k, v in page.items()}
        assert list(page) == ["id", "label", "embedding", "similarity"] and all(v.nrows == len(rows) for v in page.values())
        for name, want in zip(("id", "label", "similarity"), want_cols):
            got = page[name]
            assert got.kind == want.kind
            if name == "similarity":   # a NaN's sign and payload are the machine's
                same_floats(np.asarray(got.values).view(np.float32), want.values.view(np.float32), (form, where, page_size, page_num, name))
            else:
                same_array(np.asarray(got.values).view(np.uint8).reshape(-1), want.values.reshape(-1), (form, where, page_size, page_num, name))
            same_array(np.asarray(got.validity), want.validity, (form, name, "validity"))
            if want.offsets is not None:
                same_array(np.asarray(got.offsets), want.offsets, (form, name, "offsets"))
        got = page["embedding"]
        assert (got.layout, got.dim, got.validity_bit) == (E.FIXED, 8, 0)
        same_floats(np.asarray(got.values), want_values, (form, where, page_size, page_num, "embedding"))
        same_array(np.asarray(got.validity), want_bitmap, (form, "embedding validity"))
        assert np.asarray(page["id"].values).view(np.int64).tolist() == rows.tolist()
        # through pyarrow and back: the page's vectors and the null similarities
        arr = tabular.embedding_to_arrow(got)
        expect = [x[r].tolist() if valid[r] else None for r in rows.tolist()]
        assert arr.to_pylist() == expect
        table = tabular.columns_to_arrow({k: page[k] for k in ("id", "label", "similarity")},
                                         pa.schema([("id", pa.int64()), ("label", pa.string()), ("similarity", pa.float32())]))
        sims = table.column("similarity").to_pylist()
        assert [s is None for s in sims] == [not valid[r] for r in rows.tolist()]
        assert table.column("id").to_pylist() == rows.tolist()
        again = tabular.embedding_from_arrow(arr) if len(rows) else None
        if again is not None:
            assert [None if v is None else v.tolist() for v in E.rows(again)] == expect
    if where == "id == 42":
        first_page = chain_want(where, 100, 1)[2].tolist()
        assert first_page[0] == 300 and first_page[1:12] == [42] + list(range(100, 110))   # NaN first, then the ties in input order


@pytest.mark.parametrize("form", FORMS)
def test_nearest_neighbors_and_no_rows_found(ctx, form):
    frame, x, valid = chain_frame()
    emb = build(x, valid, E.FIXED, vbit=0)
    q = x[640].copy()
    ranked = E.similarity_exact(tabular.embedding(x, valid), q)
    rows = ranked.perm[0:50]
    if form == "host":
        page = tabular.nearest_neighbors(frame, emb, q, 50, ctx=ctx, name="score")
        ids = np.asarray(page["id"].values).view(np.int64)
        vectors = np.asarray(page["embedding"].values)
    else:
        dframe = {k: Column(c.kind, c.nrows, tensor(c.values), tensor(c.offsets), tensor(c.validity), 0, 0) for k, c in frame.items()}
        page = tabular.nearest_neighbors_device(dframe, device_embedding(emb), device_floats(q), 50, stream=ctx.stream, ctx=ctx, name="score")
        ids = page["id"].values.cpu().numpy().view(np.int64)
        vectors = page["embedding"].values.cpu().numpy()
    assert list(page) == ["id", "label", "embedding", "score"] and ids.tolist() == rows.tolist()
    same_floats(vectors, E.take(tabular.embedding(x, valid), rows)[0], (form, "vectors"))
    # a clause that selects no row, and one that selects only a row without an embedding: the reference's "no rows found"
    for where in ("id == 5000", "id == 500"):
        with pytest.raises(_capi.OxenError) as e:
            if form == "host":
                tabular.sort_by_similarity(frame, emb, where, 10, ctx=ctx)
            else:
                tabular.sort_by_similarity_device(dframe, device_embedding(emb), where, 10, stream=ctx.stream, ctx=ctx)
        assert "no rows found" in str(e.value), where
