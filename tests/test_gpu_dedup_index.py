"""The device-resident dedup index (oxen_amd/csrc/dedup_index.hip) on the GPU. The expected answer is
the dict loop below applied to the same sequence of calls; every comparison is exact."""
import filecmp
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = (1 << 64) - 1
SIZES = [0, 1, 63, 64, 65, 257, 4097, 200_000]


class Expected:
    """first[i] = seen.setdefault(key, ordinal), with the statistics counted the same way."""

    def __init__(self):
        self.seen, self.rows, self.life = {}, 0, [0, 0, 0, 0]

    def insert(self, digests, lens=None):
        first, s = np.zeros(len(digests), dtype=np.uint64), [0, 0, 0, 0]
        ln = lens.tolist() if lens is not None else None
        for i, key in enumerate(map(tuple, digests.tolist())):
            r = self.rows + i
            f = self.seen.setdefault(key, r)
            first[i] = f
            s[0 if f == r else 2] += 1
            s[1 if f == r else 3] += ln[i] if ln is not None else 0
        self.rows += len(first)
        for k, v in enumerate((s[0] + s[2], s[0], s[1] + s[3], s[1])):
            self.life[k] += v
        return first, tuple(s)

    def query(self, digests):
        return np.array([self.seen.get(key, ABSENT) for key in map(tuple, digests.tolist())], dtype=np.uint64)


def planted(n, seed):
    """n random digests, about a third of the rows copies of an earlier row: half of those of one of the
    three rows just before (near), half of any earlier row (far); copies of copies occur."""
    rng = np.random.default_rng(seed)
    dig = rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    lens = rng.integers(1, 1 << 20, size=n, dtype=np.uint64)
    if n > 1:
        rows = np.nonzero(rng.random(n) < 1 / 3)[0]
        rows = rows[rows > 0]
        near = rng.random(len(rows)) < 0.5
        src = np.where(near, rows - rng.integers(1, 4, size=len(rows)), (rng.random(len(rows)) * rows).astype(np.int64))
        for i, j in zip(rows.tolist(), np.maximum(src, 0).tolist()):
            dig[i] = dig[j]
    return dig, lens


@functools.lru_cache(maxsize=None)
def case(n, with_lens=True):
    """(digests, lens, expected first, expected stats) of one insert of planted(n) into an empty index."""
    dig, lens = planted(n, 1000 + n)
    first, stats = Expected().insert(dig, lens if with_lens else None)
    for a in (dig, lens, first):
        a.setflags(write=False)
    return dig, lens, first, stats


def life_of(stats):
    return (stats[0] + stats[2], stats[0], stats[1] + stats[3], stats[1])


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "nolens"])
@pytest.mark.parametrize("n", SIZES)
def test_first_stats_and_counts(ctx, n, with_lens):
    from oxen_amd import dedup

    dig, lens, want_first, want_stats = case(n, with_lens)
    if n >= 65:
        assert 0 < want_stats[2] < n  # the plant took: there are duplicates, and not only duplicates
    with dedup.DedupIndex(ctx) as idx:
        first, stats = idx.insert(dig, lens if with_lens else None)
        assert first.dtype == np.uint64 and np.array_equal(first, want_first)
        assert tuple(stats) == want_stats
        assert tuple(idx.counts()) == life_of(want_stats)


def test_equal_lo_or_equal_hi_are_different_keys(ctx):
    from oxen_amd import dedup

    lo_same = [(77, h) for h in range(300)]          # one start slot, told apart by hi alone
    hi_same = [(l << 20, 99) for l in range(300)]    # told apart by lo alone
    dig = np.array(lo_same + hi_same + lo_same[::-1] + hi_same[::3], dtype=np.uint64)
    want, want_stats = Expected().insert(dig)
    assert want_stats[0] == 600
    with dedup.DedupIndex(ctx) as idx:
        first, stats = idx.insert(dig)
        assert np.array_equal(first, want) and tuple(stats) == want_stats


def test_long_probe_runs(ctx):
    """5 000 distinct keys that share lo & 0xFFFF: with the table below 65 536 slots they all start at
    one slot, and above it they still start in a few."""
    from oxen_amd import dedup

    rng = np.random.default_rng(5)
    dig = np.stack([(np.arange(5000, dtype=np.uint64) << np.uint64(16)) | np.uint64(0xBEEF),
                    rng.integers(0, 1 << 64, size=5000, dtype=np.uint64)], axis=1)
    dig = np.concatenate([dig, dig[::7]])
    want, want_stats = Expected().insert(dig)
    assert want_stats[0] == 5000
    for capacity in (0, 8192):  # 131 072 and 16 384 slots
        with dedup.DedupIndex(ctx, capacity) as idx:
            first, stats = idx.insert(dig)
            assert np.array_equal(first, want) and tuple(stats) == want_stats
            assert np.array_equal(idx.query(dig[:100]), want[:100])


def test_zero_and_all_ones_are_ordinary_keys(ctx):
    from oxen_amd import dedup

    ones = (1 << 64) - 1
    dig = np.array([(0, 0), (ones, ones), (3, 4), (0, 0), (ones, ones), (0, ones), (ones, 0)], dtype=np.uint64)
    lens = np.arange(1, 8, dtype=np.uint64)
    with dedup.DedupIndex(ctx) as idx:
        assert idx.query(dig).tolist() == [ABSENT] * 7
        first, stats = idx.insert(dig, lens)
        assert first.tolist() == [0, 1, 2, 0, 1, 5, 6]
        assert tuple(stats) == (5, 1 + 2 + 3 + 6 + 7, 2, 4 + 5)
        assert idx.query(dig).tolist() == [0, 1, 2, 0, 1, 5, 6]


def test_one_key_a_hundred_thousand_times(ctx):
    from oxen_amd import dedup

    n = 100_000
    lens = np.arange(10, 10 + n, dtype=np.uint64)
    with dedup.DedupIndex(ctx) as idx:
        idx.insert(np.array([(1, 2), (3, 4), (5, 6)], dtype=np.uint64))  # so the first ordinal is not 0
        first, stats = idx.insert(np.tile(np.array([(0xABCDEF, 0x123456)], dtype=np.uint64), (n, 1)), lens)
        assert first.min() == first.max() == 3
        assert tuple(stats) == (1, 10, n - 1, int(lens[1:].sum()))
        assert tuple(idx.counts()) == (n + 3, 4, int(lens.sum()), 10)


def test_runs_of_equal_rows(ctx):
    """Runs of equal consecutive rows of every length from 1 to past three waves, at every offset within
    a wave, keys coming back in later runs and in a later call (the insert skips a row that repeats the
    row before it)."""
    from oxen_amd import dedup

    rng = np.random.default_rng(9)
    pool = rng.integers(0, 1 << 64, size=(60, 2), dtype=np.uint64)
    run_lens = np.concatenate([np.arange(1, 200), rng.integers(1, 70, size=400)])
    rng.shuffle(run_lens)
    dig = np.repeat(pool[rng.integers(0, 60, size=len(run_lens))], run_lens, axis=0)
    lens = rng.integers(1, 1 << 16, size=len(dig), dtype=np.uint64)
    cut = len(dig) // 2 + 17
    want = Expected()
    with dedup.DedupIndex(ctx, capacity=64) as idx:  # the second call grows it: the re-insert sees the runs too
        for a, b in ((0, cut), (cut, len(dig))):
            want_first, want_stats = want.insert(dig[a:b], lens[a:b])
            first, stats = idx.insert(dig[a:b], lens[a:b])
            assert np.array_equal(first, want_first) and tuple(stats) == want_stats
        assert tuple(idx.counts()) == tuple(want.life) and want.life[1] == 60


def test_several_calls_and_queries(ctx):
    from oxen_amd import dedup

    dig, lens = planted(9000, 77)
    absent = np.random.default_rng(78).integers(0, 1 << 64, size=(500, 2), dtype=np.uint64)
    parts = [(0, 1), (1, 3000), (3000, 3001), (3001, 9000)]
    want = Expected()
    with dedup.DedupIndex(ctx) as idx:
        assert np.array_equal(idx.query(dig[:1000]), want.query(dig[:1000]))  # empty index: all absent
        assert idx.query(dig[:1000]).max() == ABSENT
        for a, b in parts:
            before = tuple(idx.counts())
            probe = np.concatenate([dig[max(0, a - 200):b + 200], absent])
            assert np.array_equal(idx.query(probe), want.query(probe))
            assert tuple(idx.counts()) == before
            first, stats = idx.insert(dig[a:b], lens[a:b])
            want_first, want_stats = want.insert(dig[a:b], lens[a:b])
            assert np.array_equal(first, want_first) and tuple(stats) == want_stats
            assert tuple(idx.counts()) == tuple(want.life)
        # duplicates across calls resolved to the earlier call's ordinal
        whole, _ = Expected().insert(dig, lens)
        assert (whole[3001:] < 3001).any()
        got = idx.query(np.concatenate([dig, absent]))
        assert np.array_equal(got[:9000], whole) and (got[9000:] == ABSENT).all()
        assert tuple(idx.counts()) == tuple(want.life)
        first, stats = idx.insert(np.zeros((0, 2), dtype=np.uint64))  # n == 0 touches nothing
        assert len(first) == 0 and tuple(stats) == (0, 0, 0, 0) and tuple(idx.counts()) == tuple(want.life)


def test_growth_from_one_row(ctx):
    from oxen_amd import dedup

    dig, lens = planted(15_000, 31)
    want = Expected()
    with dedup.DedupIndex(ctx, capacity=1) as small, dedup.DedupIndex(ctx, capacity=1 << 20) as large:
        for k in range(5):
            a, b = 3000 * k, 3000 * (k + 1)
            want_first, want_stats = want.insert(dig[a:b], lens[a:b])
            for idx in (small, large):
                first, stats = idx.insert(dig[a:b], lens[a:b])
                assert np.array_equal(first, want_first) and tuple(stats) == want_stats
                assert tuple(idx.counts()) == tuple(want.life)
        assert np.array_equal(small.query(dig), want.query(dig))


def test_device_form_equals_host_form(ctx):
    import torch

    from oxen_amd import dedup

    dig, lens, want_first, want_stats = case(4097)
    d_dig = torch.from_numpy(dig.view(np.int64).copy()).to("cuda:0")
    d_lens = torch.from_numpy(lens.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    with dedup.DedupIndex(ctx) as host, dedup.DedupIndex(ctx) as dev:
        for rounds in range(2):  # the second round: every row a duplicate of the first
            h_first, h_stats = host.insert(dig, lens)
            d_first, d_stats = dev.insert_device(d_dig, d_lens, stream=ctx.stream)
            assert np.array_equal(d_first.cpu().numpy().view(np.uint64), h_first) and d_stats == h_stats
            assert dev.counts() == host.counts()
        assert np.array_equal(h_first, want_first) and h_stats == (0, 0, 4097, sum(want_stats[1::2]))
        d_first, d_stats = dev.insert_device(d_dig, None)  # no lengths, torch's current stream
        assert np.array_equal(d_first.cpu().numpy().view(np.uint64), want_first) and d_stats == (0, 0, 4097, 0)


def test_deterministic(ctx):
    from oxen_amd import dedup

    dig, lens, want_first, _ = case(200_000)
    runs = []
    for _ in range(2):
        with dedup.DedupIndex(ctx) as idx:
            runs.append(idx.insert(dig, lens)[0])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], want_first)


def test_host_forms_over_more_than_one_staged_piece(ctx):
    """The host forms stage 2^20 rows at a time: a call of 2^20 + 4 097 rows is two pieces, with
    duplicates across the seam, and answers as one insert (a later row never lowers an earlier answer)."""
    from oxen_amd import dedup

    n = (1 << 20) + 4097
    rng = np.random.default_rng(20)
    dig = rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    dig[(1 << 20) - 50:(1 << 20) + 50:2] = dig[1000:1050]     # around the seam, copies of early rows
    dig[-3000:] = dig[(1 << 20) - 3000:1 << 20]               # the second piece repeats the first one's end
    lens = rng.integers(1, 1 << 20, size=n, dtype=np.uint64)
    want_first, want_stats = Expected().insert(dig, lens)
    with dedup.DedupIndex(ctx) as idx:
        first, stats = idx.insert(dig, lens)
        assert np.array_equal(first, want_first) and tuple(stats) == want_stats
        assert tuple(idx.counts()) == life_of(want_stats)
        assert np.array_equal(idx.query(dig), want_first)


def test_fixed_size_chunks_through_the_pipeline(ctx, oracle_lib):
    from oxen_amd import dedup

    rng = np.random.default_rng(64)
    blocks = rng.integers(0, 256, size=(64, 4096), dtype=np.uint8)
    picks = rng.integers(0, 64, size=256)
    buf = np.ascontiguousarray(blocks[picks]).reshape(-1)
    assert buf.size == 1 << 20 and len(set(picks.tolist())) < 256
    tab = dedup.chunk_digests_host([buf], 4096, ctx=ctx)
    want_dig = oracle_lib.chunk_digests(buf, 4096)
    want_first, want_stats = Expected().insert(want_dig, np.full(256, 4096, dtype=np.uint64))
    with dedup.DedupIndex(ctx) as idx:
        first, stats = idx.insert(tab.digests, dedup.table_lens(tab))
        assert np.array_equal(first, want_first) and tuple(stats) == want_stats
        assert idx.counts().distinct == len(set(picks.tolist()))
    rep = dedup.dedup_report(tab)
    assert (rep["chunks"], rep["distinct_chunks"], rep["bytes"]) == (256, len(set(picks.tolist())), 1 << 20)
    assert rep["distinct_bytes"] == 4096 * len(set(picks.tolist())) and rep["files"][0]["ratio"] == rep["ratio"]


def test_fastcdc_chunks_through_the_pipeline(ctx, oracle_lib):
    from oracle import fastcdc
    from oxen_amd import dedup

    rng = np.random.default_rng(20261019)
    a, b = (rng.integers(0, 256, size=256 << 10, dtype=np.uint8) for _ in range(2))
    buf = np.concatenate([a, a, b, a])
    want_tab = fastcdc.chunks(buf, 512, 2048, 4096)
    want_dig = oracle_lib.batch(buf, want_tab[:, 0], want_tab[:, 1])
    want_first, want_stats = Expected().insert(want_dig, want_tab[:, 1].astype(np.uint64))
    assert want_stats[2] >= 1  # the cuts resynchronise inside the repeated A: duplicates exist
    tab = dedup.fastcdc_host([buf], 512, 2048, 4096, ctx=ctx)
    with dedup.DedupIndex(ctx) as idx:
        first, stats = idx.insert(tab.digests, tab.lens)
        assert np.array_equal(first, want_first) and tuple(stats) == want_stats
    with dedup.DedupIndex(ctx) as fresh:
        rep = dedup.dedup_report(tab, fresh)
        assert rep["distinct_chunks"] == want_stats[0] and rep["distinct_bytes"] == want_stats[1]
        assert rep["bytes"] == buf.size and 0 < rep["ratio"] < 1


def same_tree(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "metadata.bin" in names
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors
    return names


def repeating_file(path, seed):
    rng = np.random.default_rng(seed)
    a, b = (rng.integers(0, 256, size=256 << 10, dtype=np.uint8) for _ in range(2))
    data = np.concatenate([a, a, b, a, a[:12345]]).tobytes()
    with open(path, "wb") as fh:
        fh.write(data)
    return data


def test_fastcdc_pack_with_an_index(ctx, tmp_path):
    from oxen_amd import dedup

    src = str(tmp_path / "input.bin")
    data = repeating_file(src, 1)
    chunker = dedup.FastCDChunker(8192)
    plain = chunker.pack(src, str(tmp_path / "plain"), ctx=ctx)
    with dedup.DedupIndex(ctx) as idx:
        indexed = chunker.pack(src, str(tmp_path / "indexed"), ctx=ctx, index=idx)
        rows, distinct = idx.counts()[:2]
    names = same_tree(plain, indexed)
    assert distinct < rows and len(names) - 1 == distinct == len(set(chunker.get_chunk_hashes(indexed)))
    chunker.restore(indexed, str(tmp_path / "restored"))
    assert open(tmp_path / "restored", "rb").read() == data


def test_fixed_size_pack_with_an_index(ctx, tmp_path):
    from oxen_amd import dedup

    src = str(tmp_path / "input.bin")
    data = repeating_file(src, 2)
    chunker = dedup.FixedSizeMultiChunker(4096, 4)
    plain = chunker.pack(src, str(tmp_path / "plain"))
    with dedup.DedupIndex() as idx:  # the chunkers hash on the default context
        indexed = chunker.pack(src, str(tmp_path / "indexed"), index=idx)
        rows, distinct, nbytes, _ = idx.counts()
    names = same_tree(plain, indexed)
    assert rows == (len(data) + 4095) // 4096 and nbytes == len(data)
    assert distinct < rows and len(names) - 1 == distinct
    chunker.unpack(indexed, str(tmp_path / "restored"))
    assert open(tmp_path / "restored", "rb").read() == data


def test_directory_pack_with_one_index_for_the_output_dir(ctx, tmp_path):
    """FixedSizeChunker over a tree: files that share chunks, one index for the one output directory."""
    from oxen_amd import dedup

    tree = tmp_path / "tree"
    (tree / "sub").mkdir(parents=True)
    data = repeating_file(str(tree / "one.bin"), 3)
    (tree / "sub" / "two.bin").write_bytes(data[4096 * 5:4096 * 90] + b"tail")
    (tree / "empty").write_bytes(b"")
    chunker = dedup.FixedSizeChunker(4096)
    plain = chunker.pack(str(tree), str(tmp_path / "plain"))
    with dedup.DedupIndex() as idx:
        indexed = chunker.pack(str(tree), str(tmp_path / "indexed"), index=idx)
        rows, distinct = idx.counts()[:2]
    names = same_tree(plain, indexed)
    assert len(names) - 1 == distinct < rows
    chunker.unpack(indexed, str(tmp_path / "out"))
    assert (tmp_path / "out" / "one.bin").read_bytes() == data
    assert (tmp_path / "out" / "sub" / "two.bin").read_bytes() == data[4096 * 5:4096 * 90] + b"tail"
