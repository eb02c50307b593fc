"""The tabular kernels past their grid caps and the scan's tile loops (row_hash.hip, keyed_diff.hip,
take_columns.hip, sort_rows.hip), on the GPU.

Three edges, read from the sources below:
  G  = CAP workgroups x 256 lanes: above G rows a grid-stride kernel starts its second loop iteration
       (row_length, row_diff_mark / _flag, keyed_count / _plan / _bucket / _classify / _fill, sort_digits), and
       above G elements = 256 tiles of the scan `scan_sums_kernel` carries its total into a second batch;
  S4 = CAP tiles x kScanTile elements: above it `scan_tile_sums_kernel` and `scan_apply_kernel` loop over
       tiles; at n > S4 rows the radix pass's histogram table (256 x tiles entries) needs the scan's carry.
Every case sits at or just past one of them and compares COMPLETE outputs, exactly: with the plain-Python
restatements where they are fast enough, else with the array restatements of tests/_tabular_arrays.py,
which tests/test_tabular_arrays_cpu.py pins to the plain-Python ones."""
import functools
import os
import re

import numpy as np
import pytest

import _rowhash
import _tabular_arrays as ta
import _take
import test_keyed_diff as kd
import test_row_hash as rh
import test_sort_rows as sr
import test_take as tk
from _tabular_arrays import SIGNED
from oxen_amd import tabular
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("row_hash.hip", "keyed_diff.hip", "sort_rows.hip", "dedup_index.hip")}
CAP = 2048                                    # the most workgroups of a grid-stride launch and of the scan
SORT_TILE = int(re.search(r"constexpr uint32_t kSortTile = (\d+);", SOURCES["sort_rows.hip"]).group(1))
SCAN_PER = int(re.search(r"constexpr uint32_t kScanPer = (\d+), kScanTile = 256 \* kScanPer;", SOURCES["keyed_diff.hip"]).group(1))
SCAN_TILE = 256 * SCAN_PER
G = CAP * 256                                 # 524 288 with the shipped cap
S4 = CAP * SCAN_TILE                          # 4 194 304 with the shipped cap and tile
ROW_SHORT_MAX = int(re.search(r"constexpr uint32_t kRowShortMax = (\d+);", SOURCES["row_hash.hip"]).group(1))


def test_the_caps_the_edges_come_from():
    """A changed cap or tile fails here, loudly, instead of moving an edge away from the cases below."""
    for name in ("row_hash.hip", "keyed_diff.hip", "sort_rows.hip"):
        (cap,) = re.findall(r"unsigned stride_grid\(uint64_t n\) \{ return \(unsigned\)std::min<uint64_t>\(.*, (\d+)\); \}", SOURCES[name])
        assert int(cap) == CAP, name
    (cap,) = re.findall(r"unsigned resolve_grid\(uint64_t n\) \{ return \(unsigned\)std::min<uint64_t>\(.*, (\d+)\); \}", SOURCES["dedup_index.hip"])
    assert int(cap) == CAP
    scan = SOURCES["keyed_diff.hip"]
    scan = scan[scan.index("int exclusive_scan_u32("):]
    (cap,) = re.findall(r"const unsigned grid = \(unsigned\)std::min<uint64_t>\(std::max<uint64_t>\(ntiles, 1\), (\d+)\);", scan[:scan.index("\n}\n")])
    assert int(cap) == CAP
    assert (G, S4, SORT_TILE, SCAN_TILE) == (524288, 4194304, 2048, 2048)
    assert 256 * -(-(S4 + 2049) // SORT_TILE) > 256 * SCAN_TILE        # E3's histogram table is scanned with a carry
    assert 256 * -(-(2 * G + 1) // SORT_TILE) <= 256 * SCAN_TILE       # and E1's is not


# ---------------------------------------------------------------- A. row hashes
@functools.lru_cache(maxsize=None)
def hash_case(name):
    from oracle import oracle

    planted = {"A1": (), "A2": ((G + 100, 200),), "A3": ((G + 200, 300),), "A4": ((5, 300), (G + 5, 421))}[name]
    cols = ta.hash_frame(G + 257, planted, seed=len(planted) + ord(name[1]))
    lens = _rowhash.assemble(cols)[2].astype(np.int64)
    assert np.nonzero(lens > 12)[0].tolist() == [row for row, _ in planted] and [int(lens[row]) for row, _ in planted] == [b for _, b in planted]
    assert [b > ROW_SHORT_MAX for _, b in planted] == {"A1": [], "A2": [False], "A3": [True], "A4": [True, True]}[name]
    return cols, _rowhash.row_hashes(cols, oracle)


@pytest.mark.parametrize("form", rh.FORMS)
def test_a1_row_hashes_of_short_rows_past_the_grid(ctx, oracle_lib, form):
    """n = G + 257, every row 4-12 bytes: the rows of the length pass's second iteration."""
    rh.check(ctx, form, *hash_case("A1"))


def test_a2_the_longest_short_row_is_seen_by_the_second_iteration(ctx, oracle_lib):
    """Row G + 100 is the only row above 12 B: 200 B, still a short row, so only the second iteration of
    `row_length_kernel` knows how large the LDS slots have to be."""
    rh.check(ctx, "device", *hash_case("A2"))


def test_a3_the_only_long_row_is_seen_by_the_second_iteration(ctx, oracle_lib):
    """Row G + 200 is the only row above kRowShortMax (300 B): the long path runs only if the second
    iteration counts it."""
    rh.check(ctx, "device", *hash_case("A3"))


def test_a4_the_long_rows_of_both_iterations_add(ctx, oracle_lib):
    """Long rows at rows 5 and G + 5 (300 and 421 B): the counts and the bytes of both iterations add."""
    rh.check(ctx, "device", *hash_case("A4"))


# ---------------------------------------------------------------- B. row diff
@functools.lru_cache(maxsize=None)
def diff_case():
    base, head = ta.row_diff_keys(G // 2 + 3, G // 2 + 131, tail=300)
    removed, added, counts = ta.row_diff_arrays(base, head)
    ordinals = base.size + np.nonzero(added)[0]
    assert base.size + head.size > G and (ordinals >= G).sum() >= 134 and (ordinals < G).any() and removed[-300:].all()
    return rh.digests_of(base), rh.digests_of(head), removed, added, counts


@pytest.mark.parametrize("form", rh.FORMS)
def test_b1_row_diff_whose_rows_cross_the_grid(ctx, form):
    """G + 134 rows over both sides, the last 134 head rows -- every one of them new -- in the second
    iteration of the mark and of the flag: all flags and both counts."""
    import torch

    base, head, removed, added, counts = diff_case()
    if form == "host":
        got_added, got_removed = tabular.row_diff(base, head, ctx=ctx)
        assert np.array_equal(got_added, np.nonzero(added)[0]) and np.array_equal(got_removed, np.nonzero(removed)[0])
        assert (got_removed.size, got_added.size) == counts
        return
    d_base = torch.from_numpy(base.view(np.int64).copy()).to("cuda:0")
    d_head = torch.from_numpy(head.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    got_added, got_removed, got_counts = tabular.row_diff_device(d_base, d_head, stream=ctx.stream, ctx=ctx)
    assert np.array_equal(got_added.cpu().numpy(), added) and np.array_equal(got_removed.cpu().numpy(), removed)
    assert got_counts == (counts[1], counts[0])


# ---------------------------------------------------------------- C. keyed diff
@pytest.mark.parametrize("form", kd.FORMS)
@pytest.mark.parametrize("keep", [False, True], ids=["changed", "all"])
def test_c1_keyed_diff_whose_rows_cross_the_grid(ctx, form, keep):
    """nl + nr = G + 65 rows: the count, the plan, the classify and the fill reach their second iteration,
    whose six counters add to the first's."""
    case = kd.size_case(G // 2 + 1, G // 2 + 64)
    want, counts, dupes = kd.check(ctx, form, case, keep)
    assert dupes == (0, 0) and all(counts[s] > G // 40 for s in counts)


@functools.lru_cache(maxsize=None)
def split_case():
    left, right, lt, rt, groups = ta.dupes_split_case(4099, G + 257, G)
    for kind, (a, b), key, rows in groups:
        assert np.array_equal(np.nonzero(right == key)[0], rows) and (rows.min() >= G if kind == "past" else rows.min() < G <= rows.max())
    return kd.Case(kd.digests_of(left), kd.digests_of(right), kd.digests_of(lt), kd.digests_of(rt))


@pytest.mark.parametrize("form", kd.FORMS)
def test_c2_duplicate_groups_on_both_sides_of_right_row_G(ctx, form):
    """nr = G + 257: the only case in which `keyed_bucket_kernel` has a second iteration. Groups of (left,
    right) multiplicity (1, 2), (2, 3) and (1, 65) with every right row past right row G, and (1, 2), (2, 3),
    (1, 65) and (1, 300) with right rows on both sides of it, two equal neighbours at G - 1 and G among
    them. (A (1, 300) group cannot lie past G: there are 257 rows.)"""
    want, counts, dupes = kd.check(ctx, form, split_case(), keep=True)
    assert dupes == (2 * 2, 2 * (2 + 3 + 65) + 300)


@functools.lru_cache(maxsize=None)
def scan_case():
    return ta.keyed_int_case(S4 // 2 + 1, S4 // 2 + 2048)


@pytest.mark.parametrize("keep", [False, True], ids=["changed", "all"])
def test_c3_keyed_diff_whose_scan_loops_over_tiles(ctx, keep):
    """nl + nr = S4 + 2 049 rows: the scan of emit[] runs over 2 050 tiles -- more than its grid, and nine
    batches of tile sums. Unique keys, a fifth of the rows dropped, added and modified; most emit words are
    0 without the unchanged pairs and 1 with them."""
    import torch

    (lrows, rrows, status), counts, dupes = ta.keyed_diff_arrays(*scan_case(), keep)
    assert -(-(S4 + 2049) // SCAN_TILE) == CAP + 2
    emitted = lrows.size / (S4 + 2049)
    assert emitted > 0.6 if keep else emitted < 0.35
    dev = [kd.on_device(kd.digests_of(a)) for a in scan_case()]
    torch.cuda.synchronize()
    d = tabular.keyed_diff_digests_device(*dev, keep_unchanged=keep, stream=ctx.stream, ctx=ctx)
    assert (d.added, d.removed, d.modified, d.unchanged) == (counts[ta.ADDED], counts[ta.REMOVED], counts[ta.MODIFIED], counts[ta.UNCHANGED])
    assert (d.dupes_left, d.dupes_right) == dupes
    assert np.array_equal(d.left_rows.cpu().numpy(), lrows.astype(np.int32))
    assert np.array_equal(d.right_rows.cpu().numpy(), rrows.astype(np.int32))
    assert np.array_equal(d.status.cpu().numpy(), status)


# ---------------------------------------------------------------- D. take
def check_take(ctx, form, case):
    cols, idx0, idx1, plan = case
    want = _take.take(cols, idx0, idx1, plan)
    got = tk.python_call(ctx, form, list(cols), idx0, idx1, plan)
    tk.same(got, want)
    assert int(got[1].offsets[-1]) == int(want[1].offsets[-1]) == want[1].values.size
    return want


@pytest.mark.parametrize("form", tk.FORMS)
def test_d1_take_whose_offsets_carry_past_256_tiles(ctx, form):
    """nout = G + 1: the lengths fill 257 tiles of the scan, so the last tile's offsets stand on the carry
    of `scan_sums_kernel`. Output rows 0 and G select a 5 000 B cell: a long piece lands after the carry, at
    an offset that holds the first one's bytes."""
    want = check_take(ctx, form, ta.take_case(G + 1, big_at=(0, G)))
    lens = np.diff(want[1].offsets.astype(np.int64))
    assert lens[0] == lens[G] == ta.BIG_CELL and int(want[1].offsets[G]) > ta.BIG_CELL + G


def test_d2_take_whose_scan_loops_over_tiles(ctx):
    """nout = S4 + 2 049: 2 050 tiles of lengths 0-7, real numbers, not flags."""
    want = check_take(ctx, "device", ta.take_case(S4 + 2049))
    assert int(want[1].offsets[-1]) > 2 * (S4 + 2049)


# ---------------------------------------------------------------- E. sort
def sorted_by(ctx, form, cols, orders=None):
    cols = [c if isinstance(c, Column) else Column(c.dtype.itemsize, c.size, c) for c in cols]
    perm, stats = sr.run(ctx, form, cols, [SIGNED] * len(cols) if orders is None else orders)
    assert perm.dtype == np.uint32
    return perm, stats


def same_perm(perm, want):
    assert perm.shape == want.shape
    if not np.array_equal(perm, want):
        at = int(np.nonzero(perm != want)[0][0])
        raise AssertionError(("first difference at place", at, perm[at:at + 4].tolist(), want[at:at + 4].tolist()))


@pytest.mark.parametrize("n,form", [(G, "device"), (G + 1, "device"), (G + 1, "host"), (2 * G + 1, "device")])
def test_e1_sort_of_random_keys_around_the_grid(ctx, n, form):
    """`sort_digits_kernel` ends its first iteration at row G - 1; one row and a whole second launch past it."""
    keys = ta.int64_keys(n)
    perm, stats = sorted_by(ctx, form, [keys])
    same_perm(perm, np.argsort(keys, kind="stable").astype(np.uint32))
    assert (stats.rounds, stats.passes, stats.tied) == (1, 8, 0)


@pytest.mark.parametrize("byte", [0, 3, 7])
def test_e2_the_one_mark_of_the_second_iteration_in_a_word_digit(ctx, byte):
    """n = G + 1, every key equal but the last row's, whose byte `byte` is lower: the one mark that makes
    that digit's pass necessary comes from the second iteration of `sort_digits_kernel`."""
    n = G + 1
    perm, stats = sorted_by(ctx, "device", [ta.one_low_row(n, byte)])
    same_perm(perm, np.concatenate([[n - 1], np.arange(n - 1)]).astype(np.uint32))
    assert (stats.rounds, stats.passes, stats.tied) == (1, 1, n - 1)


@pytest.mark.parametrize("which", ["class digit", "tail digit"])
def test_e2_the_one_mark_of_the_second_iteration_in_a_meta_digit(ctx, which):
    """The same for the digits of `meta`: every row valid but the last, which is null; b"abc" everywhere
    but b"ab" in the last row."""
    n = G + 1
    col = ta.one_null_row(n) if which == "class digit" else ta.one_short_row(n)
    perm, stats = sorted_by(ctx, "device", [col])
    same_perm(perm, np.concatenate([[n - 1], np.arange(n - 1)]).astype(np.uint32))
    assert stats.passes >= 1


def test_e3_sort_whose_histogram_scan_carries_one_key(ctx):
    """n = S4 + 2 049 = 2 050 tiles: the histogram table has 524 800 entries, so its scan carries, and the
    flag scan loops over tiles."""
    n = S4 + 2049
    keys = ta.int64_keys(n)
    want, tied = ta.sort_indices_arrays([Column(8, n, keys)])
    assert np.array_equal(want, np.argsort(keys, kind="stable"))
    perm, stats = sorted_by(ctx, "device", [keys])
    same_perm(perm, want)
    assert (stats.rounds, stats.passes, stats.tied) == (1, 8, tied)


def test_e3_sort_whose_histogram_scan_carries_two_keys(ctx):
    """The same rows by an int32 key of 100 000 values with a third of the rows null (validity_bit 5), then
    a random int64 key: round 2 sorts by group ids that fill three bytes of `meta`."""
    n = S4 + 2049
    first, second = ta.grouped_keys(n, 100000)
    assert first.validity_bit == 5 and np.unique(first.values).size > 65536
    want, tied = ta.sort_indices_arrays([first, second])
    perm, stats = sorted_by(ctx, "device", [first, second])
    same_perm(perm, want)
    assert stats.rounds == 2 and stats.tied == tied
