"""Every leasing entry under a poison: no result may depend on what a call's working memory held before.

Each entry of the library works in memory it does not initialise as a whole -- one of the device's two cached
scratch buffers and its pinned words (ScratchLease, csrc/scratch.hpp), a CallBlock (csrc/columns.hpp), the blocks
it allocates for itself -- and zeroes or 0xFF-fills exactly the parts it must. The suite inherits those bytes from
the test before, in a fixed order, and a fresh allocation is usually zero; oxh_set_scratch_poison fills every such
allocation with a byte of the test's choosing before the call uses it. 0x00 and 0xFF are both "empty" somewhere
(the bucket and dedup tables, kGroupEmpty, OXH_TAKE_NULL, the control words), so a missing fill of one kind passes
under the byte that equals it; 0x5A equals neither. Every case compares COMPLETE outputs exactly, through the
owning module's helpers, with expected values computed once for the three bytes, and requires
oxh_scratch_poisoned_bytes() to have grown around the calls: an entry that is no longer wired fails.

What initialises each region, read from the sources (csrc/<entry>.hip). "written part" = only what the call wrote
is read back.
  row hashes    CallBlock d [cols | ctrl 8]          one copy of the whole pinned half (zeroed, the columns set)
                lease long_row / long_off / long_len  memset 0 (3 * nlong words), then row_long_plan_kernel
                lease digests 2 * nlong               K1 over the arena writes every one; the scatter reads those
                lease arena long_bytes + 256          row_long_gather_kernel writes [off, off + len) of every long
                                                      row; K1 reads the items' own bytes (written part)
                host block [digests | columns]        the pieces are copied up; the digests are written for every row
  row diff      block first n                         the index's resolve writes every row's first ordinal
                block ctrl 4 | last 2n                memset 0
                pinned ctrl 4                         one copy of all 4 words down
                host block [digests 2n | flags n]     copies up; row_diff_flag_kernel writes every flag
  keyed diff    block id n                            the two inserts' resolves write every row
                block off n | scan sums tiles + 1     exclusive_scan_u32 writes all of both (sums[ntiles] included)
                block ctrl 8                          memset 0
                block grp 4n                          memset 0
                block emit n                          keyed_classify_kernel writes every row
                block bucket nr                       memset 0xFF
                pinned ctrl 8                         one copy of all 8 words down
                host in block / out block             copies up / keyed_fill_kernel writes counts8[0] pairs (written part)
  take          CallBlock d [src | out | ctrl | totals]  measure copies [src | out | ctrl] (ctrl 0 from the pinned half);
                                                      write copies [src | out] again and, without byte columns, memsets
                                                      ctrl; the totals words of the device half are never used
                lease len n / off n / sums tiles + 1  take_resolve_kernel<false> writes every len; the scan the rest
                d_lists npieces * 12                  memset 0xFF, then take_long_plan_kernel
                host in block / out block             copies up / every validity byte, offset and value byte in use is written
  sort          CallBlock d [cols | ctrl]             copy of the columns; ctrl memset 0 at every round
                lease places[0]                       sort_init_kernel writes the four arrays
                lease places[1]                       sort_apply_kernel writes the four arrays before a round reads them
                lease word / meta / order[0]          sort_keys_kernel, every row, every round
                lease order[1] / keys[0..1]           a radix pass (or the gather) writes all n before the next reads
                lease flag / flag_scan / sums         sort_flag_kernel every row; the scan
                lease table / table_scan              radix_hist_kernel writes all 256 * tiles entries; the scan
                host block [perm | columns]           copies up; perm is a copy of places[cur].row
  group rows    CallBlock d (images) / ctrl block     as the row hashes' / memset 0
                lease digests / first                 the hash kernels write every row / the insert's resolve
                lease count_of n                      memset 0
                lease flag n                          group_count_kernel writes every row
                lease flag_scan / sums                the scan
                lease long rows' scratch              as the row hashes'
                host block [4 outputs | columns]      copies up; written part
  filter rows   lease ctrl                            memset 0
                lease lits                            copy of the literal words in use; the kernel reads lit_words of them
                lease counts / mask blocks            filter_eval_kernel writes every block
                lease bases / sums                    the scan
                pinned [lits | ctrl]                  memcpy of the literals; the ctrl words are copied down
                host block [idx | mask | columns]     copies up; written part (idx: `selected` entries)
  embedding     lease ctrl 8                          memset 0, first-wrong memset 0xFF
                lease partial groups * dim (mean)     emb_mean_partial_kernel: every workgroup writes its whole row
                pinned ctrl                           one copy of all words down
                host block                            copies up; the outputs in front are written part
                similarity's sort                     its own lease, as the sort above
  concat        lease / pinned [probes | answers]     memcpy + copy up of the probes; the kernel writes every answer
                lease / pinned write block            row_base, bits, dst, spans, items by memcpy, ctrl memset 0 on the
                                                      pinned side, one copy of all of it up (the gaps are not read)
                host in block / out block             copies up / every byte of the outputs' sizes is written
  dedup index   d_keys                                rows [0, rows + n) by copies; nothing past them is read
                d_table (create, growth)              memset 0xFF
                d_ctrl / h_ctrl                       memset 0 at every call / one copy of all 8 words down
                piece buffers                         memcpy + copy of the m rows in use (written part)
  chunk overlap block first (| lens)                  the resolve writes every row (| copies up)
                block member | matrix | error word    memset 0
                block set_first / pinned tail         memcpy + copy up; the matrix and the error word are copied down
  K1L           lease block sums, two rounds          xxh3_blocksum_kernel writes the nb sums a chain then reads
                lease state 8 per buffer              the chain of round 0 (not kChainResume) writes it before round 1 reads
                oversize item's buffer                copy of the item; the results area at its end by a copy
  FastCDC       lease foff / flen / sec_base          copies up
                lease sec_file / first                cdc_sec_file_kernel / cdc_first_kernel, every entry
                lease cand, cand_occ (scan)           F1 writes every section's occupancy and the candidates it counts
                lease entry (walk)                    the walk writes every section's entry before X reads it
                lease spec / spec_cnt                 F2 (or W) writes spec_cnt and the starts below it (written part)
                lease status / k0                     cdc_check_kernel (or X), every section
                lease count / exit                    the check where it converged, the fix-up everywhere else
                lease fix                             written part (read only where status is kFixed)
                lease out_base                        cdc_prefix_kernel writes all n_sec + 1
"""
import contextlib
import functools

import numpy as np
import pytest

import _cdc_plant as P
import _concat
import _embedding as E
import _filterrows as F
import _grouprows
import _rowhash
import _sortrows
import _tabular_arrays as ta
import _take
import test_concat as cc
import test_embedding as em
import test_filter_rows as fr
import test_gpu_chunk_overlap as co
import test_gpu_dedup_index as di
import test_gpu_lattice as lat
import test_group_rows as gr
import test_keyed_diff as kd
import test_row_hash as rh
import test_sort_rows as sr
import test_take as tk
from _tabular_arrays import SIGNED
from oracle import fastcdc as CDC
from oxen_amd import _capi
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu

POISONS = [0x00, 0xFF, 0x5A]


@pytest.fixture(params=POISONS, ids=["0x00", "0xFF", "0x5A"])
def poison(request, ctx):
    L = _capi.lib()
    prev = L.oxh_set_scratch_poison(request.param)
    try:
        assert prev == -1, prev
        yield request.param
    finally:
        L.oxh_set_scratch_poison(-1)


@contextlib.contextmanager
def poisoned(what):
    """The calls inside must have filled some working memory: a case whose counter stands still is not wired."""
    L = _capi.lib()
    before = L.oxh_scratch_poisoned_bytes()
    yield
    assert L.oxh_scratch_poisoned_bytes() > before, (what, "no working allocation was poisoned")


def test_the_switch_itself(ctx):
    L = _capi.lib()
    assert L.oxh_set_scratch_poison(-1) == -1
    assert L.oxh_set_scratch_poison(0x5A) == -1 and L.oxh_set_scratch_poison(256) == 0x5A    # out of range: off
    assert L.oxh_set_scratch_poison(-7) == -1 and L.oxh_set_scratch_poison(-1) == -1
    before = L.oxh_scratch_poisoned_bytes()
    rh.check_diff(ctx, "device", [1, 2, 3], [2, 3, 4])
    assert L.oxh_scratch_poisoned_bytes() == before                                           # off: nothing is filled


# ---------------------------------------------------------------- row hashes and the row diff
@functools.lru_cache(maxsize=None)
def hash_case():
    from oracle import oracle

    cols = ta.hash_frame(4099, ((5, 300), (4000, 421)), seed=3)
    lens = _rowhash.assemble(cols)[2]
    assert sorted(int(x) for x in lens[lens > rh_short_max()]) == [300, 421]
    return cols, _rowhash.row_hashes(cols, oracle)


def rh_short_max():
    import test_tabular_past_grid as past

    return past.ROW_SHORT_MAX


@pytest.mark.parametrize("form", rh.FORMS)
def test_row_hashes_with_two_long_rows(ctx, oracle_lib, poison, form):
    """4 099 rows of 4-12 B and two above kRowShortMax: the arena, the three lists of long rows and the cursor words."""
    with poisoned("row hashes"):
        rh.check(ctx, form, *hash_case())


@functools.lru_cache(maxsize=None)
def diff_case():
    base, head = ta.row_diff_keys(3001, 3003, tail=100)
    base, head = rh.digests_of(base), rh.digests_of(head)
    want = _rowhash.compute_new_row_indices(_rowhash.hex_strings(base), _rowhash.hex_strings(head))
    assert len(want[0]) >= 100 and len(want[1]) >= 100
    return base, head, want


@pytest.mark.parametrize("form", rh.FORMS)
def test_row_diff(ctx, poison, form):
    base, head, want = diff_case()
    with poisoned("row diff"):
        got = rh.diff(ctx, form, base, head)
    assert got == want, (got[0][:8], want[0][:8], got[1][:8], want[1][:8])


# ---------------------------------------------------------------- keyed diff
@pytest.mark.parametrize("form", kd.FORMS)
@pytest.mark.parametrize("keep", [False, True], ids=["changed", "all"])
@pytest.mark.parametrize("case", ["dupes", "two scan tiles"])
def test_keyed_diff(ctx, poison, case, keep, form):
    """Buckets and groups; 4 160 rows, more than one tile of the scan, so its sums are read."""
    c = kd.dupes_case() if case == "dupes" else kd.size_case(2049, 2111)
    with poisoned("keyed diff"):
        want, counts, dupes = kd.check(ctx, form, c, keep)
    assert (dupes != (0, 0)) == (case == "dupes") and len(want) > 100


# ---------------------------------------------------------------- take
@functools.lru_cache(maxsize=None)
def take_cases():
    cells = tk.threshold_cells(np.random.default_rng(8))
    order = np.arange(len(cells), dtype=np.uint32)
    long_pieces = ([tk.strings(cells, lead=b"q"), tk.strings(cells, _take.BYTES64)], order[::-1].copy(), order,
                   [(0, 0, None, 0), (1, 1, None, 0), (1, 0, None, 0)])
    return {"long pieces": long_pieces, "4099 rows": ta.take_case(4099, big_at=(0, 4098))}


@functools.lru_cache(maxsize=None)
def take_want(name):
    cols, i0, i1, plan = take_cases()[name]
    return _take.take(list(cols), i0, i1, plan)


@pytest.mark.parametrize("form", tk.FORMS)
@pytest.mark.parametrize("name", ["long pieces", "4099 rows"])
def test_take(ctx, poison, name, form):
    """Cells around the threshold and the piece size (the item lists); 4 099 output rows with two 5 000 B cells."""
    cols, i0, i1, plan = take_cases()[name]
    with poisoned("take"):
        got = tk.python_call(ctx, form, list(cols), i0, i1, plan)
    tk.same(got, take_want(name))


# ---------------------------------------------------------------- sort
@functools.lru_cache(maxsize=None)
def sort_cases():
    rng = np.random.default_rng(12)
    first, second = ta.grouped_keys(9 * sr.T + 1, 300)
    cells = [b"p" * 20 + bytes(rng.integers(97, 100, size=int(l), dtype=np.uint8)) for l in rng.integers(0, 12, size=700)]
    return {"two keys": [first, second], "prefix": [sr.strings(cells, lead=b"LEAD!")]}


@functools.lru_cache(maxsize=None)
def sort_want(name):
    cols = sort_cases()[name]
    return _sortrows.sort_indices(cols, [SIGNED] * len(cols)) if name == "prefix" else ta.sort_indices_arrays(cols)


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("name", ["two keys", "prefix"])
def test_sort(ctx, poison, name, form):
    """9 tiles and a row by an int32 key with nulls, then an int64 one: two rounds, skipped passes, both sets of
    places and both key buffers. Strings that share 20 bytes: the chunk cursors, three rounds and more."""
    cols = sort_cases()[name]
    want, tied = sort_want(name)
    with poisoned("sort"):
        perm, stats = sr.run(ctx, form, cols, [SIGNED] * len(cols))
    assert perm.dtype == np.uint32 and perm.shape == want.shape
    if not np.array_equal(perm, want):
        at = int(np.nonzero(perm != want)[0][0])
        raise AssertionError((form, "first difference at place", at, perm[at:at + 4].tolist(), want[at:at + 4].tolist()))
    assert stats.tied == tied and stats.rounds >= (2 if name == "two keys" else 3), stats


# ---------------------------------------------------------------- group rows
@functools.lru_cache(maxsize=None)
def group_cases():
    frame = gr.mixed_frame()
    names = ["i8", "f32", "i64", "b", "s", "ls"]
    n = 9 * gr.SCAN_TILE + 1
    rng = np.random.default_rng(13)
    labels = [b"label-%03d" % k for k in rng.integers(0, 100, size=n).tolist()]
    labels[n // 2] = b"L" * 400                                       # one long row
    return {"mixed": ([frame[x] for x in names], [gr.MIXED_ORDERS[x] for x in names]),
            "labels": ([gr.strings(labels)], [SIGNED])}


@functools.lru_cache(maxsize=None)
def group_want(name):
    return _grouprows.group_rows(*group_cases()[name])


@pytest.mark.parametrize("form", gr.FORMS)
@pytest.mark.parametrize("name", ["mixed", "labels"])
def test_group_rows(ctx, poison, name, form):
    cols, orders = group_cases()[name]
    want = group_want(name)
    assert want.stats[1] > 0 and (name != "labels" or want.stats[:1] + want.stats[3:] == (101, 1))    # one long row
    with poisoned("group rows"):
        got = gr.run(ctx, form, cols, orders)
    gr.same(got, want, form)


# ---------------------------------------------------------------- filter rows
@functools.lru_cache(maxsize=None)
def filter_terms_case():
    frame = fr.kinds_frame()
    names = ["i32", "f64", "bytes32"]
    cols, orders = [frame[x][0] for x in names], [frame[x][1] for x in names]
    terms = [(0, F.GE, frame["i32"][2][1]), (1, F.LT, frame["f64"][2][2]), (2, F.EQ, b"ab")]
    logical = [F.OR, F.AND]
    want = F.filter_rows(cols, terms, logical, orders)
    assert 0 < want.stats[0] < cols[0].nrows and want.stats[1] > 0
    return cols, terms, logical, orders, want


@functools.lru_cache(maxsize=None)
def filter_blocks_case():
    n = 64 * fr.SCAN_TILE + 65
    values = np.random.default_rng(14).integers(-128, 128, size=n, dtype=np.int8)
    want = fr.array_selection(values, F.LT, -64)
    assert -(-n // 64) == fr.SCAN_TILE + 2 and n // 5 < want.stats[0] < n // 3
    return values, want


@pytest.mark.parametrize("form", fr.FORMS)
def test_filter_rows_three_terms(ctx, poison, form):
    cols, terms, logical, orders, want = filter_terms_case()
    with poisoned("filter rows"):
        got = fr.raw_call(ctx, form, cols, terms, logical, orders)
    fr.same(got, want, (form, "three terms"))


@pytest.mark.parametrize("form", fr.FORMS)
def test_filter_rows_two_scan_tiles_of_block_counts(ctx, poison, form):
    values, want = filter_blocks_case()
    with poisoned("filter rows"):
        got = fr.raw_call(ctx, form, [fr.column(values)], [(0, F.LT, (-64) & 0xFF)])
    fr.same(got, want, (form, values.size))


# ---------------------------------------------------------------- embedding
@functools.lru_cache(maxsize=None)
def embedding_cases():
    rng = np.random.default_rng(15)
    x, valid = em.integers(rng, 600, 257), em.some_valid(rng, 600)
    idx = np.sort(rng.choice(600, 257, replace=False)).astype(np.uint32)
    mean = (em.build(x, valid, E.LIST32, 1, 3, first=2), idx, em.exact_mean(x, valid, idx))
    x, valid = em.integers(rng, 130, 17), em.some_valid(rng, 130)
    q = rng.integers(-8, 9, size=17).astype(np.float32)
    sim = (em.build(x, valid, E.FIXED, 3, 7), q, em.exact_want(x, valid, q))
    x, valid = em.integers(rng, 200, 17), em.some_valid(rng, 200)
    take_idx = rng.integers(0, 200, 65).astype(np.uint32)
    take_idx[rng.random(65) < 0.2] = E.TAKE_NULL
    emb = em.build(x, valid, E.LIST64, 2, 3, first=1)
    take = (emb, take_idx, E.take(emb, take_idx))
    return mean, sim, take


@pytest.mark.parametrize("form", em.FORMS)
def test_embedding_mean(ctx, poison, form):
    """dim 257 over 257 indices: five workgroups' partial rows, two tiles across dim. Integer values: exact."""
    (emb, idx, (want, stats)), _, _ = embedding_cases()
    assert em.MEAN_GROUPS >= 5 and -(-257 // em.MEAN_CHUNK) == 5
    with poisoned("embedding mean"):
        got = em.mean_call(ctx, form, emb, idx)
    em.same_mean(got, want, stats, (form, "mean"))


@pytest.mark.parametrize("form", em.FORMS)
def test_embedding_similarity_with_keys_and_perm(ctx, poison, form):
    """The sort's lease right after the similarity's, on the same buffer."""
    _, (emb, q, want), _ = embedding_cases()
    with poisoned("embedding similarity"):
        got = em.similarity_call(ctx, form, emb, q)
    em.same_similarity(got, want, (form, "similarity"))


@pytest.mark.parametrize("form", em.FORMS)
def test_embedding_take(ctx, poison, form):
    _, _, (emb, idx, (values, bitmap, stats)) = embedding_cases()
    with poisoned("embedding take"):
        got = em.take_call(ctx, form, emb, idx)
    assert got.rc == em.OK and got.stats == stats, (form, got.rc, got.stats, stats)
    em.same_floats(got.out, values, (form, "take"))
    em.same_array(got.validity, bitmap, (form, "take validity"))


@functools.lru_cache(maxsize=None)
def random_mean_case():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((5000, 768)).astype(np.float32)
    valid = em.some_valid(rng, 5000)
    idx = np.sort(rng.choice(5000, 3000, replace=False)).astype(np.uint32)
    return em.build(x, valid, E.LIST32, 3, 3, 2), idx


MEAN_BITS = {}     # form -> (poison, the bits of the first poison's mean)


@pytest.mark.parametrize("form", em.FORMS)
def test_random_mean_has_the_same_bits_under_every_poison(ctx, poison, form):
    """Random normal data, where the order of the additions and a stale partial row would show."""
    emb, idx = random_mean_case()
    with poisoned("embedding mean"):
        got = em.mean_call(ctx, form, emb, idx)
    assert got.rc == em.OK and got.stats[0] > 2000
    first_poison, bits = MEAN_BITS.setdefault(form, (poison, got.out.view(np.uint32).copy()))
    em.same_array(got.out.view(np.uint32), bits, (form, "poison", hex(poison), "against", hex(first_poison)))


# ---------------------------------------------------------------- concat
@functools.lru_cache(maxsize=None)
def concat_case():
    rng = np.random.default_rng(16)
    parts = [cc.frame(rng, n, [1, 4, 8, 16, 32, 64], bit) for n, bit in ((70, 0), (131, 3), (257, 5))]
    ranges = [(3, 60), (0, 131), (5, 200)]
    return parts, ranges, _concat.concat(parts, ranges)


@pytest.mark.parametrize("form", cc.FORMS)
def test_concat(ctx, poison, form):
    """Three parts of every kind with ranges: the measure's lease block, then the write's in the same lease."""
    parts, ranges, want = concat_case()
    with poisoned("concat"):
        got = cc.raw_call(ctx, form, parts, ranges, cc.sizes_of(want))
    cc.assert_same(got, want, form)


# ---------------------------------------------------------------- dedup index and chunk overlap
@functools.lru_cache(maxsize=None)
def growth_case():
    dig, lens = di.planted(15_000, 31)
    want, steps = di.Expected(), []
    for k in range(5):
        steps.append(want.insert(dig[3000 * k:3000 * (k + 1)], lens[3000 * k:3000 * (k + 1)]))
    return dig, lens, steps, want.query(dig), tuple(want.life)


def test_dedup_index_grows_from_one_row(ctx, poison):
    """Five inserts into an index made for one row -- a new key store and a new table where it grows -- then a query."""
    from oxen_amd import dedup

    dig, lens, steps, want_query, life = growth_case()
    L = _capi.lib()
    with poisoned("dedup index"):
        with dedup.DedupIndex(ctx, capacity=1) as idx:
            for k, (want_first, want_stats) in enumerate(steps):
                before = L.oxh_scratch_poisoned_bytes()
                first, stats = idx.insert(dig[3000 * k:3000 * (k + 1)], lens[3000 * k:3000 * (k + 1)])
                assert np.array_equal(first, want_first) and tuple(stats) == want_stats, k
                if k < 3:      # 1 -> 3 000 -> 6 000 -> 12 000 rows of room
                    assert L.oxh_scratch_poisoned_bytes() > before, k
            assert tuple(idx.counts()) == life
            assert np.array_equal(idx.query(dig), want_query)


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "nolens"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_chunk_overlap(ctx, poison, form, with_lens):
    sets, lens, want_rows, want_bytes = co.case((300, 257, 64))
    with poisoned("chunk overlap"):
        got = co.run(ctx, form, sets, lens if with_lens else None)
    co.check(got, want_rows, want_bytes if with_lens else None)


# ---------------------------------------------------------------- K1L
@pytest.fixture(scope="module")
def k1l_arena(cuda):
    import torch

    from oxen_amd.device import fill_splitmix

    arena = torch.empty(lat.K1L_SPAN, dtype=torch.uint8, device=cuda)
    fill_splitmix(arena, 79)
    return arena, arena.cpu().numpy()


def test_k1l_69_chained_buffers(cuda, ctx, oracle_lib, k1l_arena, poison):
    """nb = 1025 at every residue and three shifts: the chain launch flushes mid-round (kChainJobs = 32)."""
    arena, host = k1l_arena
    items = [(s, 1025 * 1024 + r) for s in lat.K1L_SHIFTS for r in lat.K1L_R]
    assert len(items) == 69
    with poisoned("K1L"):
        lat._check_k1l(oracle_lib, arena, host, items, "K1L nb 1025 under a poison")


def test_k1l_resumed_chains(cuda, ctx, oracle_lib, poison, monkeypatch):
    """1 MiB pieces: the chains of the second and third piece resume from accumulators that live in the lease."""
    import torch

    from oxen_amd.device import fill_splitmix

    monkeypatch.setenv("OXH_BIG_PIECE_MIB", "1")
    piece = 1 << 20
    sizes = [piece + d for d in (1, 1023, 1024, 1025, 1026)] + [2 * piece + 1024, 2 * piece + 1025, 3 * piece + 7]
    arena = torch.empty(3 * piece + 64, dtype=torch.uint8, device=cuda)
    fill_splitmix(arena, 80)
    with poisoned("K1L pieces"):
        lat._check_k1l(oracle_lib, arena, arena.cpu().numpy(), [(5, n) for n in sizes], "K1L 1 MiB pieces under a poison")


@pytest.fixture(scope="module")
def big_files(tmp_path_factory, oracle_lib):
    from oxen_amd.workloads import splitmix_bytes

    paths = []
    for i in range(3):
        p = tmp_path_factory.mktemp("scratch_contents") / f"big{i}.bin"
        p.write_bytes(splitmix_bytes(90 + i, 0, (3 << 20) + 5000).tobytes())
        paths.append(str(p))
    out, _, _ = oracle_lib.hash_files(paths, threads=3)
    return paths, [(int(hi) << 64) | int(lo) for lo, hi in out]


def test_large_files_through_one_mib_pieces(cuda, poison, big_files, monkeypatch):
    """Three files above a 1 MiB staging slot, side by side through the large-item pipeline in 1 MiB pieces."""
    from oxen_amd import hasher

    monkeypatch.setenv("OXH_BIG_PIECE_MIB", "1")
    paths, want = big_files
    with poisoned("large files"):
        with _capi.Context(0, staging_bytes=1 << 20) as c:
            digests, sizes, status = hasher.hash_files_128bit(paths, c)
    assert all(s == 0 for s in status) and sizes == [(3 << 20) + 5000] * 3
    assert digests == want


# ---------------------------------------------------------------- device FastCDC
# the smallest parameters of tests/_cdc_plant.py's configs, and the smallest of those the walk takes
CDC_CASES = {"scan": ((64, 256, 1024), [300, 517, 900], [411, 1000]), "walk": ((4096, 4096, 8192), [4300, 5000, 7000], [4200, 6100])}


@functools.lru_cache(maxsize=None)
def cdc_case(path):
    from oracle import oracle

    cfg, cuts, more = CDC_CASES[path]
    assert cfg in (P.WALK_CONFIGS if path == "walk" else P.CONFIGS)
    pl = P.plant(cfg, 1, [P.Random(until=1 << 20)] + cuts + [P.Random(until=3 << 20)] + more, seed=9, size_hint=4 << 20)
    want = CDC.chunks(pl.data, *cfg)
    assert not pl.absent and want[:, 1].tolist() == pl.lens and len(pl.data) > 3 << 20
    offs, lens = want[:, 0].astype(np.uint64), want[:, 1].astype(np.uint64)
    return cfg, pl.data, offs, lens, oracle.batch(pl.data, offs, lens, threads=8)


@pytest.mark.parametrize("path", ["scan", "walk"])
def test_fastcdc_device(cuda, ctx, oracle_lib, poison, path, monkeypatch):
    """One planted buffer of 3 MiB per chunking path (OXH_CDC_WALK; the walk fails loudly where it cannot be taken):
    boundaries against the chunk oracle, digests against the hash oracle."""
    import torch

    from oxen_amd.device import fastcdc_device, to_numpy_u64

    for knob in ("OXH_CDC_SECTION_BYTES", "OXH_CDC_WARMUP_BYTES", "OXH_CDC_UNIT_CAP"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("OXH_CDC_WALK", "1" if path == "walk" else "0")
    cfg, data, offs, lens, want_dig = cdc_case(path)
    d_arena = torch.from_numpy(data).to(cuda)
    with poisoned("fastcdc"):
        c_off, c_len, dig, first = fastcdc_device(d_arena, np.zeros(1, np.uint64), np.array([data.size], np.uint64), *cfg, 1)
    assert first.tolist() == [0, offs.size]
    assert np.array_equal(to_numpy_u64(c_off), offs) and np.array_equal(to_numpy_u64(c_len), lens)
    assert np.array_equal(to_numpy_u64(dig).reshape(-1, 2), want_dig)
