"""The stable multi-column row sort on the GPU (oxh_sort_rows_*, oxen_amd/csrc/sort_rows.hip;
oxen_amd.tabular): the permutation of both forms is compared for EXACT equality with the restatement of
tests/_sortrows.py -- Python's stable `sorted` over tuple keys -- everywhere, and stats3[2] with its count of
the rows that equal another row on every key."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import _rowhash
import _sortrows
import _take
from _sortrows import FLOAT, SIGNED, UNSIGNED
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
SOURCE = open(os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc", "sort_rows.hip")).read()
T = int(re.search(r"constexpr uint32_t kSortTile = (\d+);", SOURCE).group(1))   # the shipped tile of the radix pass


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


def run(ctx, form, cols, orders):
    import torch

    if form == "host":
        perm, stats = tabular.sort_indices(cols, orders, ctx=ctx)
        return perm, stats
    dev = [device_column(c) for c in cols]
    torch.cuda.synchronize()
    perm, stats = tabular.sort_indices_device(dev, orders, stream=ctx.stream, ctx=ctx)
    assert perm.is_cuda and perm.dtype == torch.int32
    return perm.cpu().numpy().view(np.uint32), stats


def check(ctx, cols, orders=None, forms=FORMS):
    """Both forms against the restatement; returns the stats of the last form."""
    cols = [c if isinstance(c, Column) else column(c) for c in cols]
    orders = [SIGNED] * len(cols) if orders is None else list(orders)
    want, tied = _sortrows.sort_indices(cols, orders)
    stats = None
    for form in forms:
        perm, stats = run(ctx, form, cols, orders)
        assert perm.dtype == np.uint32 and perm.shape == want.shape
        if not np.array_equal(perm, want):
            at = int(np.nonzero(perm != want)[0][0])
            raise AssertionError((form, "first difference at place", at, perm[at:at + 4].tolist(), want[at:at + 4].tolist()))
        assert stats.tied == tied, (form, stats, tied)
        assert stats.rounds >= 1
    return stats


def strings(cells, kind=_take.BYTES32, valid=None, bit=0, lead=b""):
    """A byte column from a list of bytes: `lead` bytes before the first cell (so offsets[0] != 0), the
    validity bitmap's row 0 at `bit`. A null cell keeps its bytes underneath, as Arrow allows."""
    off = np.zeros(len(cells) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cells], out=off[1:])
    data = np.frombuffer(lead + b"".join(cells), dtype=np.uint8)
    offsets = (off + len(lead)).astype(np.int32 if kind == _take.BYTES32 else np.int64)
    return Column(kind, len(cells), data, offsets, None if valid is None else _rowhash.packed_at(valid, bit), 0,
                  0 if valid is None else bit)


def with_nulls(c, rng, bit=5):
    """A third of the rows null, the validity bitmap's row 0 at `bit`."""
    return c._replace(validity=_rowhash.packed_at(rng.random(c.nrows) > 1 / 3, bit), validity_bit=bit)


# ---------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 9 * T + 1, 2**18 + 3])
def test_sizes_with_random_int64_keys(ctx, n):
    """Around a wave, around a tile, ten tiles -- where the histogram table of 256 x tiles outgrows one
    2 048-element tile of the scan -- and many tiles."""
    keys = np.random.default_rng(n).integers(-2**63, 2**63, size=n).astype(np.int64)
    stats = check(ctx, [keys])
    assert stats.rounds == 1 and stats.tied == 0 and stats.passes <= 8
    if n > T:
        assert stats.passes == 8   # every byte of thousands of random words takes more than one value


# ---------------------------------------------------------------- 2. stability and skipped passes
def test_stability_and_skipped_passes(ctx):
    n = 3 * T + 17
    rng = np.random.default_rng(2)
    same = np.full(n, 0x0123456789ABCDEF, dtype=np.int64)
    stats = check(ctx, [same])                                  # every digit has a single value: no pass at all
    assert stats == (1, 0, n)
    perm, _ = run(ctx, "device", [column(same)], [SIGNED])
    assert np.array_equal(perm, np.arange(n, dtype=np.uint32))
    two = np.where(rng.random(n) < 0.5, 7, -7).astype(np.int64)  # two values: stable inside each
    assert check(ctx, [two]).tied == n
    top = (rng.integers(0, 256, size=n).astype(np.int64) << 56) | 0x00AA55AA55AA55AA    # only the top byte differs
    assert check(ctx, [top], [UNSIGNED]).passes == 1
    low = rng.integers(0, 256, size=n).astype(np.int64) | 0x7711223344556600             # only the low byte
    assert check(ctx, [low]).passes == 1
    every = np.tile(np.arange(256, dtype=np.int64), T // 256)                            # all 256 values of one digit in one tile
    every = every[rng.permutation(every.size)] << 16
    stats = check(ctx, [every])
    assert stats.passes == 1 and stats.tied == every.size


# ---------------------------------------------------------------- 3. kinds
KIND_CASES = {
    "int8": (lambda rng, n: np.concatenate([[-128, 127, 0, -1], rng.integers(-128, 128, size=n - 4)]).astype(np.int8), SIGNED),
    "int32": (lambda rng, n: np.concatenate([[-2**31, 2**31 - 1], rng.integers(-2**31, 2**31, size=n - 2)]).astype(np.int32), SIGNED),
    "uint32": (lambda rng, n: np.concatenate([[0, 2**32 - 1, 2**31, 2**31 - 1], rng.integers(0, 2**32, size=n - 4)]).astype(np.uint32), UNSIGNED),
    "float32": (lambda rng, n: np.concatenate([[np.inf, -np.inf, 0.0, -0.0], rng.standard_normal(n - 4)]).astype(np.float32), FLOAT),
    "int64": (lambda rng, n: np.concatenate([[-2**63, 2**63 - 1, 0, -1], rng.integers(-2**63, 2**63, size=n - 4)]).astype(np.int64), SIGNED),
    "uint64": (lambda rng, n: np.concatenate([np.array([0, 2**64 - 1, 2**63, 2**63 - 1], dtype=np.uint64),
                                              rng.integers(0, 2**64, size=n - 4, dtype=np.uint64)]), UNSIGNED),
    "float64": (lambda rng, n: np.concatenate([[np.inf, -np.inf, 1.7976931348623157e308, -1.7976931348623157e308],
                                               rng.standard_normal(n - 4)]), FLOAT),
}


@pytest.mark.parametrize("name", list(KIND_CASES))
def test_fixed_width_kinds_with_nulls(ctx, name):
    """Every width in its order classes, the extremes included; validity_bit 5 and a third of the rows null:
    the nulls come first and keep their order."""
    n = T + 301
    rng = np.random.default_rng(len(name))
    make, order = KIND_CASES[name]
    values = make(rng, n)
    c = Column(values.dtype.itemsize, n, values)
    check(ctx, [c], [order])
    nulls = with_nulls(c, rng)
    stats = check(ctx, [nulls], [order])
    valid = _rowhash.bits(nulls.validity, 5, n)
    perm, _ = run(ctx, "device", [nulls], [order])
    k = int((~valid).sum())
    assert np.array_equal(perm[:k], np.nonzero(~valid)[0]) and stats.tied >= k > n // 4
    # a narrow repeat: many ties, broken by nothing -- input order
    few = values[rng.integers(0, 5, size=n)]
    check(ctx, [Column(values.dtype.itemsize, n, few)], [order])


@pytest.mark.parametrize("bit", [3, 13])
def test_booleans(ctx, bit):
    n = T + 77
    rng = np.random.default_rng(bit)
    mask = rng.random(n) < 0.5
    c = Column(16, n, _rowhash.packed_at(mask, bit), None, None, bit, 0)
    stats = check(ctx, [c])
    assert stats.tied == n and stats.passes == 1
    perm, _ = run(ctx, "host", [c], [SIGNED])
    assert np.array_equal(perm, np.concatenate([np.nonzero(~mask)[0], np.nonzero(mask)[0]]))
    check(ctx, [with_nulls(c, rng)], [77])           # the order class of a boolean is ignored


# ---------------------------------------------------------------- 4. floats
def test_float_order(ctx):
    """±0.0 interleaved and tied, in input order; ±inf; subnormals; NaNs of different payload and sign tied and
    last."""
    nan64 = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                      0xFFF5A5A5A5A5A5A5], dtype=np.uint64).view(np.float64)
    special = np.concatenate([[0.0, -0.0] * 8, [np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
                                                1e-310, -1e-310, 1.0, -1.0], nan64, [-0.0, 0.0], nan64[::-1]])
    rng = np.random.default_rng(4)
    f = np.concatenate([special, rng.standard_normal(T)])[rng.permutation(special.size + T)]
    stats = check(ctx, [f], [FLOAT])
    assert stats.tied == 18 + 12
    perm, _ = run(ctx, "device", [column(f)], [FLOAT])
    assert np.isnan(f[perm[-12:]]).all() and np.array_equal(perm[-12:], np.nonzero(np.isnan(f))[0])
    zeros = np.nonzero(f == 0)[0]
    at = int(np.nonzero(perm == zeros[0])[0][0])
    assert np.array_equal(perm[at:at + 18], zeros)
    nan32 = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFA55AA5], dtype=np.uint32).view(np.float32)
    g = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39], dtype=np.float32), nan32,
                        rng.standard_normal(300).astype(np.float32)])   # float32 throughout: the payloads stay
    assert g.dtype == np.float32 and np.array_equal(g[7:13].view(np.uint32), nan32.view(np.uint32))
    check(ctx, [g[rng.permutation(g.size)]], [FLOAT])
    check(ctx, [with_nulls(column(f), rng)], [FLOAT])


# ---------------------------------------------------------------- 5. several keys
def test_several_keys(ctx):
    n = 2 * T + 9
    rng = np.random.default_rng(5)
    four = rng.integers(0, 4, size=n).astype(np.int32)
    wide = rng.integers(-2**63, 2**63, size=n).astype(np.int64)
    stats = check(ctx, [four, wide])                                   # round 2 sorts by the group id as well
    assert stats.rounds == 2 and stats.tied == 0
    # three keys, a null in the first broken by the second; the third never looked at where the second decides
    a = with_nulls(column(rng.integers(0, 3, size=n).astype(np.int8)), rng)
    b = column(rng.integers(0, 50, size=n).astype(np.int32))
    c = column(rng.standard_normal(n))
    stats = check(ctx, [a, b, c], [SIGNED, SIGNED, FLOAT])
    assert stats.rounds == 3
    # a unique first key decides everything in one round, whatever follows
    unique = rng.permutation(n).astype(np.int64)
    words = strings([bytes(rng.integers(97, 100, size=int(l), dtype=np.uint8)) for l in rng.integers(0, 30, size=n)])
    stats = check(ctx, [unique, words])
    assert stats.rounds == 1 and stats.tied == 0
    flags = Column(16, n, _rowhash.packed_at(rng.random(n) < 0.5, 3), None, None, 3, 0)
    stats = check(ctx, [with_nulls(flags, rng), np.round(rng.standard_normal(n), 1)], [SIGNED, FLOAT])
    assert stats.rounds == 2 and stats.tied > 0


# ---------------------------------------------------------------- 6. strings
def random_cells(rng, n, alphabet=(97, 100)):
    lens = rng.choice([0, 1, 3, 7, 8, 9, 15, 16, 17, 24, 40], size=n, p=[.05, .05, .05, .15, .15, .15, .1, .1, .1, .05, .05])
    return [bytes(rng.integers(*alphabet, size=int(l), dtype=np.uint8)) for l in lens]


def expected_rounds(cells, valid=None):
    present = [c for k, c in enumerate(cells) if valid is None or valid[k]]
    return _sortrows.byte_rounds(present) if present else 1


def test_string_lengths_around_the_chunk(ctx):
    """Lengths 0-40, dense around 7, 8, 9, 15, 16 and 17, over a three-letter alphabet: many ties per chunk."""
    rng = np.random.default_rng(6)
    n = T + 501
    cells = random_cells(rng, n)
    stats = check(ctx, [strings(cells)])
    assert stats.rounds == expected_rounds(cells) and stats.tied > 0
    valid = rng.random(n) > 1 / 3
    col = strings(cells, valid=valid, bit=5, lead=b"LEAD!")             # offsets[0] != 0, validity_bit 5
    assert col.offsets[0] == 5
    assert check(ctx, [col]).rounds == expected_rounds(cells, valid)
    check(ctx, [strings(cells[::-1], _take.BYTES64, valid, 5)])          # int64 offsets


def test_string_ladder_and_high_bytes(ctx):
    ladder = [b"b", b"a\0\0", b"a", b"", b"a\0", b"a\0\0", b"", b"a", b"\x80", b"\x7f", b"\xff\xfe", b"\xff", b"a\0\0\0\0\0\0\0", b"a\0\0\0\0\0\0\0\0"]
    valid = np.ones(len(ladder) + 2, dtype=bool)
    valid[[3, len(ladder)]] = False
    col = strings(ladder + [b"zz", b""], valid=valid, bit=5)
    perm, stats = run(ctx, "device", [col], [SIGNED])
    want, tied = _sortrows.sort_indices([col])
    assert perm.tolist() == want.tolist() and stats.tied == tied
    assert perm[:2].tolist() == [3, len(ladder)] and perm[2:4].tolist() == [6, len(ladder) + 1]   # nulls, then the empty cells
    check(ctx, [col])
    rng = np.random.default_rng(7)
    check(ctx, [strings(random_cells(rng, 700, alphabet=(0x7E, 0x83)))])    # bytes on both sides of 0x80


def test_long_common_prefix_costs_rounds_only_while_tied(ctx):
    rng = np.random.default_rng(8)
    shorts = [bytes(rng.integers(97, 123, size=int(l), dtype=np.uint8)) for l in rng.integers(1, 7, size=200)]
    prefix = [b"p" * 64 + bytes([97 + k % 7]) for k in range(40)]
    cells = shorts + prefix
    stats = check(ctx, [strings(cells)])
    assert stats.rounds == _sortrows.byte_rounds(cells) == 9           # 8 full chunks of the prefix, then byte 64
    # two 5 000-byte cells that differ in their last byte, among short ones
    big = bytes(rng.integers(0, 256, size=4999, dtype=np.uint8))
    cells = shorts[:60] + [big + b"\x02", big + b"\x01"] + shorts[60:120]
    stats = check(ctx, [strings(cells)], forms=["device"])
    assert stats.rounds == _sortrows.byte_rounds(cells) == 625
    # one 5 000-byte cell that is unique in its first word: the rounds the short cells need, no more
    cells = shorts + [b"\xf0unique!" + big]
    stats = check(ctx, [strings(cells)])
    assert stats.rounds == _sortrows.byte_rounds(shorts) == _sortrows.byte_rounds(cells) and stats.rounds <= 2


# ---------------------------------------------------------------- 7. what the device refuses
def test_decreasing_offsets_on_the_device_form(ctx):
    """A decreasing pair of offsets is a cell of length 0 and OXH_ERR_INVALID; nothing outside a named span is
    read, and the process goes on."""
    import torch

    good = column(["ab", "cd", "ef", "g", ""])
    broken = good._replace(offsets=np.array([0, 2, 4, 3, 7, 7], dtype=np.int32))   # a decreasing pair at row 2
    dev = device_column(broken)
    perm = torch.full((5,), 9, dtype=torch.int32, device="cuda:0")
    stats = np.full(3, 7, dtype=np.uint64)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    rc = _capi.lib().oxh_sort_rows_device(ctx.handle, 5, 1, *tabular._tables([dev], ptr), (ctypes.c_uint32 * 1)(0), perm.data_ptr(),
                                          stats.ctypes.data_as(_capi._u64p), ctx.stream)
    assert rc == _capi.OXH_ERR_INVALID and b"offsets" in _capi.lib().oxh_last_error()
    assert stats.tolist() == [7, 7, 7]
    with pytest.raises(_capi.OxenError, match="decrease"):
        tabular.sort_indices([broken], ctx=ctx)                # the host form reads the offsets itself
    check(ctx, [good])                                          # and the next call is fine


# ---------------------------------------------------------------- 8. the diff, sorted
def as_taken(c):
    host = lambda x: None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))  # noqa: E731
    assert c.value_bit == 0 and c.validity_bit == 0 and c.validity is not None
    return _take.Taken(c.kind, c.nrows, host(c.values).view(np.uint8).reshape(-1), host(c.offsets), host(c.validity))


def same(got, want):
    assert len(got) == len(want)
    for o, (g, w) in enumerate(zip(got, want)):
        assert g.kind == w.kind and g.nrows == w.nrows, o
        assert np.array_equal(g.validity, w.validity), ("validity", o, g.kind)
        assert (g.offsets is None) == (w.offsets is None)
        if w.offsets is not None:
            assert g.offsets.dtype == w.offsets.dtype and np.array_equal(g.offsets, w.offsets), ("offsets", o, g.kind)
        assert np.array_equal(g.values, w.values), ("values", o, g.kind)


@functools.lru_cache(maxsize=None)
def diff_frames(case):
    """Two frames of a few thousand rows whose keys are unique on each side: int keys, string keys, or
    (str, int) with nulls in keys[1]."""
    n = 3000
    rng = np.random.default_rng(90 + len(case))
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    names = ["k%05d" % i for i in rng.permutation(n)]
    score = np.round(rng.standard_normal(n), 2)
    left = {"id": column(ids), "name": column(names), "score": column(score)}
    keep = rng.permutation(n)[: n - 200]
    r_score = score[keep].copy()
    r_score[rng.random(keep.size) < 0.2] += 1.0
    extra = 150
    r_ids = np.concatenate([ids[keep], 10 * n + rng.permutation(extra)]).astype(np.int64)
    r_names = [names[i] for i in keep] + ["new%04d" % i for i in rng.permutation(extra)]
    right = {"name": column(r_names), "score": column(np.concatenate([r_score, np.zeros(extra)])), "id": column(r_ids)}
    if case == "str_int_nulls":   # names repeat in pairs; the id, null here and there, tells them apart
        left["name"] = column(["k%05d" % (int(x[1:]) // 2) for x in names])
        right["name"] = column(["k%05d" % (int(x[1:]) // 2) if x[0] == "k" else x for x in r_names])
        left["id"] = column(ids, validity=rng.random(n) > 0.05)
        right["id"] = column(r_ids, validity=np.concatenate([np.asarray(_rowhash.bits(left["id"].validity, 0, n))[keep], np.ones(extra, bool)]))
    return left, right


@pytest.mark.parametrize("case,keys", [("int", ["id"]), ("str", ["name"]), ("str_int_nulls", ["name", "id"])])
def test_diff_dfs_contents_sorted(ctx, case, keys):
    """`diff_dfs_contents(sort=True)`: the rows are the unsorted call's rows in the restatement's order of the
    keys' coalesce(right, left) columns, and every buffer of the contents is the restatement's take through
    them."""
    left, right = diff_frames(case)
    d0, plain = tabular.diff_dfs_contents(left, right, keys=keys, targets=["score"], ctx=ctx)
    d, contents = tabular.diff_dfs_contents(left, right, keys=keys, targets=["score"], ctx=ctx, sort=True)
    assert list(contents) == list(plain) and len(d0.left_rows) > 300
    sources = list(left.values()) + list(right.values())
    key_plan = tabular._sort_key_plan(left, right, keys)
    key_cols = [Column(t.kind, t.nrows, t.values, t.offsets, t.validity) for t in _take.take(sources, d0.left_rows, d0.right_rows, key_plan)]
    perm, _ = _sortrows.sort_indices(key_cols, [SIGNED] * len(keys))
    assert np.array_equal(d.left_rows, d0.left_rows[perm]) and np.array_equal(d.right_rows, d0.right_rows[perm])
    assert np.array_equal(d.status, d0.status[perm]) and d[3:] == d0[3:]
    assert not np.array_equal(perm, np.arange(perm.size))
    wanted = tabular.output_columns(left, right, keys, ["score"])
    where = {("left", n): i for i, n in enumerate(left)}
    where.update({("right", n): len(left) + i for i, n in enumerate(right)})
    side = {"left": 0, "right": 1}
    plan = [(where[a], side[a[0]], None if b is None else where[b], 0 if b is None else side[b[0]]) for _, a, b in wanted]
    same([as_taken(contents[w[0]]) for w in wanted], _take.take(sources, d.left_rows, d.right_rows, plan))
    assert _take.pylist(contents["_oxen_diff_status"]) == [tabular.STATUS_NAMES[s] for s in d.status.tolist()]
    # a list of names: the last key alone
    d1, _ = tabular.diff_dfs_contents(left, right, keys=keys, targets=["score"], ctx=ctx, sort=keys[-1:])
    perm1, _ = _sortrows.sort_indices(key_cols[-1:], [SIGNED])
    assert np.array_equal(d1.left_rows, d0.left_rows[perm1])


def test_sorted_diff_on_the_device_with_a_repeated_key(ctx):
    """The device steps (`sort_diff_rows_device`) after `keyed_diff_digests_device`. A key that repeats on the
    right comes out of the device diff in any order, so inside each run of equal keys the multiset of rows is
    compared; the keys themselves come in order."""
    import torch

    rng = np.random.default_rng(12)
    n = 2000
    ids = rng.permutation(n).astype(np.int64)
    left = {"id": column(ids), "v": column(rng.integers(0, 9, size=n).astype(np.int32))}
    r_ids = np.concatenate([ids[rng.permutation(n)[:1500]], ids[:40], ids[:40], n + np.arange(100)]).astype(np.int64)   # 40 keys three times
    right = {"id": column(r_ids), "v": column(rng.integers(0, 9, size=r_ids.size).astype(np.int32))}
    dl = {k: device_column(c) for k, c in left.items()}
    dr = {k: device_column(c) for k, c in right.items()}
    torch.cuda.synchronize()
    on = lambda f, names: tabular.row_hashes_device([c for k, c in f.items() if k in names], stream=ctx.stream, ctx=ctx)  # noqa: E731
    d0 = tabular.keyed_diff_digests_device(on(dl, ["id"]), on(dr, ["id"]), on(dl, ["v"]), on(dr, ["v"]), keep_unchanged=True,
                                           stream=ctx.stream, ctx=ctx)
    d = tabular.sort_diff_rows_device(dl, dr, d0, ["id"], orders=[SIGNED], stream=ctx.stream, ctx=ctx)
    assert d.left_rows.is_cuda and d.status.is_cuda and d.left_rows.numel() == d0.left_rows.numel()
    l, r, s = (t.cpu().numpy() for t in (d.left_rows, d.right_rows, d.status))
    l0, r0, s0 = (t.cpu().numpy() for t in (d0.left_rows, d0.right_rows, d0.status))
    key = np.where(r >= 0, r_ids[np.maximum(r, 0)], ids[np.maximum(l, 0)])
    assert (np.diff(key) >= 0).all() and key.size > n
    assert sorted(zip(key.tolist(), l.tolist(), r.tolist(), s.tolist())) == \
        sorted(zip(np.where(r0 >= 0, r_ids[np.maximum(r0, 0)], ids[np.maximum(l0, 0)]).tolist(), l0.tolist(), r0.tolist(), s0.tolist()))
    # stable: inside a run of equal keys the rows keep the order the diff wrote them in
    place0 = {pair: i for i, pair in enumerate(zip(l0.tolist(), r0.tolist()))}
    order = np.array([place0[pair] for pair in zip(l.tolist(), r.tolist())])
    assert all((np.diff(order[key == k]) > 0).all() for k in ids[:40].tolist())
    got = tabular.take_device([dl["v"], dr["v"]], d.left_rows, d.right_rows, [(0, 0, None, 0), (1, 1, None, 0)], stream=ctx.stream, ctx=ctx)
    same([as_taken(g) for g in got], _take.take([left["v"], right["v"]], l, r, [(0, 0, None, 0), (1, 1, None, 0)]))


def test_sort_by_one_column_of_each_kind(ctx):
    n = 1500
    rng = np.random.default_rng(13)
    frame = {"i8": column(rng.integers(-128, 128, size=n).astype(np.int8)), "f32": column(rng.standard_normal(n).astype(np.float32)),
             "i64": with_nulls(column(rng.integers(-2**63, 2**63, size=n).astype(np.int64)), rng, bit=0),
             "b": column(rng.random(n) < 0.5), "s": column(["w%d" % (i % 97) for i in rng.permutation(n)]),
             "ls": strings([b"x" * int(l) for l in rng.integers(0, 20, size=n)], _take.BYTES64)}
    cols = list(frame.values())
    for name, c in frame.items():
        got = tabular.sort_by(frame, name, ctx=ctx)
        assert list(got) == list(frame)
        perm, _ = _sortrows.sort_indices([c], [FLOAT if name == "f32" else SIGNED])
        same([as_taken(g) for g in got.values()], _take.take(cols, perm))
    with pytest.raises(_capi.OxenError, match="not in the frame"):
        tabular.sort_by(frame, "ghost", ctx=ctx)
