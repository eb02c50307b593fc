"""Row hashes of a frame from its columns and the row diff on the GPU (oxh_row_hashes_*, oxh_row_diff_*,
oxen_amd/csrc/row_hash.hip; oxen_amd.tabular). Every digest is compared, exactly, with the restatement
of tests/_rowhash.py -- numpy row assembly by the row-bytes rule, hashed by the C oracle -- through both
the host and the device form; every diff with the dict-based compute_new_row_indices written as
repositories/diffs.rs:1023-1074 writes it. Parity with polars' own bytes is restated from the cited
lines, not pinned."""
import functools

import numpy as np
import pytest

import _rowhash
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]


def on_device(a):
    import torch

    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def run(ctx, form, cols):
    """(n, 2) uint64 digests of the frame through one form of the call."""
    import torch

    if form == "host":
        return tabular.row_hashes(cols, ctx=ctx)
    dev = [c._replace(values=on_device(c.values), offsets=on_device(c.offsets), validity=on_device(c.validity)) for c in cols]
    torch.cuda.synchronize()
    out = tabular.row_hashes_device(dev, stream=ctx.stream, ctx=ctx)
    return out.cpu().numpy().view(np.uint64)


def check(ctx, form, cols, want):
    got = run(ctx, form, cols)
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


def text_column(lengths, seed, kind=32, lead=0):
    """A byte column whose row r has lengths[r] random bytes; `lead` bytes of noise before the first
    (offsets[0] = lead, a sliced string array)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    values = rng.integers(0, 256, size=lead + int(offsets[-1]) + 3, dtype=np.uint8)   # and 3 bytes after the last
    offsets += lead
    return Column(kind, lengths.size, values, offsets.astype(np.int32 if kind == 32 else np.int64))


# ---------------------------------------------------------------- 1. length classes
LENGTHS = list(range(301)) + [1023, 1024, 1025, 4097]


@functools.lru_cache(maxsize=None)
def length_case(with_int8):
    from oracle import oracle

    cols = [text_column(LENGTHS, 11)]
    if with_int8:  # every string then starts one byte off in its row
        cols.insert(0, column(np.arange(len(LENGTHS), dtype=np.int64).astype(np.int8)))
    return cols, _rowhash.row_hashes(cols, oracle)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_int8", [False, True], ids=["text", "int8+text"])
def test_length_classes(ctx, oracle_lib, form, with_int8):
    """Row r is r bytes long for r = 0..300, so the rows cross every XXH3 class edge (0, 1-3, 4-8, 9-16,
    17-128, 129-240) and rows 240 and 241 -- the last short and the first long one -- are neighbouring
    lanes of one wave; then 1 023, 1 024, 1 025 and 4 097 bytes."""
    cols, want = length_case(with_int8)
    lens = _rowhash.assemble(cols)[2].astype(np.int64)
    assert lens[:301].tolist() == [r + with_int8 for r in range(301)] and (lens > 240).sum() >= 60
    assert tuple(int(v) for v in want[0]) == (oracle_lib.xxh3_128(b"") if not with_int8 else oracle_lib.xxh3_128(b"\x00"))
    check(ctx, form, cols, want)


# ---------------------------------------------------------------- 2. all kinds in one frame
@functools.lru_cache(maxsize=None)
def kinds_frame():
    n = 257
    rng = np.random.default_rng(5)
    f32 = rng.standard_normal(n).astype(np.float32)
    f64 = rng.standard_normal(n)
    f32[[3, 100]], f64[[4, 200]] = (np.nan, -0.0), (np.nan, -0.0)
    lengths = rng.integers(0, 40, size=n)
    return {
        "i8": column(rng.integers(-128, 128, size=n).astype(np.int8)),
        "i32": column(rng.integers(-2**31, 2**31, size=n).astype(np.int32)),
        "i64": column(rng.integers(-2**63, 2**63, size=n, dtype=np.int64)),
        "f32": column(f32), "f64": column(f64),
        "b": column(rng.random(n) < 0.5),
        "s32": text_column(lengths, 21, 32),
        "s64": text_column(lengths, 21, 64),
    }


@pytest.mark.parametrize("form", FORMS)
def test_all_kinds_in_one_frame(ctx, oracle_lib, form):
    frame = kinds_frame()
    assert [c.kind for c in frame.values()] == [1, 4, 8, 4, 8, 16, 32, 64]
    order_a = list(frame)
    order_b = ["s64", "b", "f64", "i8", "s32", "i64", "f32", "i32"]
    got = {}
    for key, order in (("a", order_a), ("b", order_b)):
        cols = [frame[k] for k in order]
        want = _rowhash.row_hashes(cols, oracle_lib)
        got[key] = want
        check(ctx, form, cols, want)   # each permutation equals the restatement for its own order
    assert (got["a"] != got["b"]).any(axis=1).all()   # and the order matters, row by row
    # BYTES32 and BYTES64 of the same strings give equal digests
    a, b = run(ctx, form, [frame["i32"], frame["s32"]]), run(ctx, form, [frame["i32"], frame["s64"]])
    assert np.array_equal(a, b) and np.array_equal(a, _rowhash.row_hashes([frame["i32"], frame["s32"]], oracle_lib))


# ---------------------------------------------------------------- 3. nulls and bit offsets
@functools.lru_cache(maxsize=None)
def null_frame(bit0):
    """Every kind with a validity bitmap whose row 0 is bit `bit0`; the boolean's values start there too.
    Row 7 is null in every column; the strings sit behind 5 bytes of noise (offsets[0] = 5)."""
    n = 131
    rng = np.random.default_rng(100 + bit0)

    def valid():
        m = rng.random(n) < 0.7
        m[7] = False
        m[8] = True
        return _rowhash.packed_at(m, bit0, rng)

    def with_nulls(c, value_bit=0):
        return c._replace(validity=valid(), validity_bit=bit0, value_bit=value_bit)

    truth = rng.random(n) < 0.5
    return [
        with_nulls(column(rng.integers(-128, 128, size=n).astype(np.int8))),
        with_nulls(column(rng.integers(-2**31, 2**31, size=n).astype(np.int32))),
        with_nulls(column(rng.integers(-2**63, 2**63, size=n, dtype=np.int64))),
        with_nulls(column(rng.standard_normal(n).astype(np.float32))),
        with_nulls(column(rng.standard_normal(n))),
        with_nulls(Column(16, n, _rowhash.packed_at(truth, bit0, rng)), value_bit=bit0),
        with_nulls(text_column(rng.integers(0, 30, size=n), 31 + bit0, 32, lead=5)),
        with_nulls(text_column(rng.integers(0, 30, size=n), 41 + bit0, 64, lead=5)),
    ]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bit0", [0, 1, 7, 9])
def test_nulls_and_bit_offsets(ctx, oracle_lib, form, bit0):
    cols = null_frame(bit0)
    assert int(cols[6].offsets[0]) == 5 and cols[5].value_bit == bit0
    want = _rowhash.row_hashes(cols, oracle_lib)
    rows = _rowhash.row_bytes(cols)
    assert rows[7] == b"" and rows[8] != b"" and len({len(r) for r in rows}) > 10
    assert tuple(int(v) for v in want[7]) == oracle_lib.xxh3_128(b"")   # null in every column: the empty input
    check(ctx, form, cols, want)
    check(ctx, form, cols[5:6], _rowhash.row_hashes(cols[5:6], oracle_lib))   # the boolean column alone


# ---------------------------------------------------------------- 4. row counts
@functools.lru_cache(maxsize=None)
def count_case(n):
    from oracle import oracle

    rng = np.random.default_rng(n)
    cols = [column(rng.integers(-2**31, 2**31, size=n).astype(np.int32)), text_column(rng.integers(0, 9, size=n), n + 1)]
    return cols, _rowhash.row_hashes(cols, oracle)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100003])
def test_row_counts(ctx, form, n):
    cols, want = count_case(n)
    check(ctx, form, cols, want)


def test_no_rows_is_ok_and_touches_nothing(ctx):
    empty = [column(np.zeros(0, dtype=np.int64)), column([])]
    assert tabular.row_hashes(empty, ctx=ctx).shape == (0, 2)


def test_decreasing_offsets_on_the_device_are_an_error_not_a_read(ctx):
    """The device form cannot see the offsets before the launch: a decreasing pair is a cell of length 0 and
    the call comes back with OXH_ERR_INVALID. (The values are large enough that the pair names bytes inside
    them whichever way it is read.)"""
    c = Column(32, 3, np.arange(64, dtype=np.uint8), np.array([0, 9, 4, 12], dtype=np.int32))
    with pytest.raises(_capi.OxenError) as e:
        run(ctx, "device", [c])
    assert e.value.code == _capi.OXH_ERR_INVALID and "decrease" in str(e.value)
    with pytest.raises(_capi.OxenError) as e:
        run(ctx, "host", [c])
    assert e.value.code == _capi.OXH_ERR_INVALID


# ---------------------------------------------------------------- 5. diff
def digests_of(keys):
    """(n, 2) digests that are equal exactly where the integer keys are."""
    k = np.asarray(keys, dtype=np.uint64)
    return np.stack([k * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1), k ^ np.uint64(0xC2B2AE3D27D4EB4F)], axis=1)


def diff(ctx, form, base, head):
    """(added, removed) as ascending index lists through one form."""
    import torch

    if form == "host":
        added, removed = tabular.row_diff(base, head, ctx=ctx)
        assert added.dtype == np.uint32 and removed.dtype == np.uint32
        return added.tolist(), removed.tolist()
    d_base = torch.from_numpy(base.view(np.int64).copy()).to("cuda:0")
    d_head = torch.from_numpy(head.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    added, removed, counts = tabular.row_diff_device(d_base, d_head, stream=ctx.stream, ctx=ctx)
    added, removed = added.cpu().numpy(), removed.cpu().numpy()
    assert set(np.unique(added)) <= {0, 1} and set(np.unique(removed)) <= {0, 1}
    assert counts == (int(added.sum()), int(removed.sum()))
    return np.nonzero(added)[0].tolist(), np.nonzero(removed)[0].tolist()


def check_diff(ctx, form, base_keys, head_keys):
    base, head = digests_of(base_keys), digests_of(head_keys)
    want = _rowhash.compute_new_row_indices(_rowhash.hex_strings(base), _rowhash.hex_strings(head))
    got = diff(ctx, form, base, head)
    assert got == want, (got[0][:8], want[0][:8], got[1][:8], want[1][:8])
    return want


@pytest.mark.parametrize("form", FORMS)
def test_diff_reports_the_last_occurrence(ctx, form):
    # key 5 is three times in base and not in head; key 9 twice in head and not in base; 1 and 2 in both
    added, removed = check_diff(ctx, form, [5, 1, 5, 2, 5, 1], [9, 1, 2, 9, 2])
    assert removed == [4] and added == [3]    # a first-occurrence answer would be [0] and [0]


@pytest.mark.parametrize("form", FORMS)
def test_diff_edges(ctx, form):
    rng = np.random.default_rng(17)
    keys = rng.integers(0, 1 << 60, size=300).tolist()
    assert check_diff(ctx, form, keys, keys) == ([], [])                                  # head == base
    other = [k + (1 << 61) for k in keys[:257]]
    assert check_diff(ctx, form, keys, other) == (list(range(257)), list(range(300)))     # disjoint
    assert check_diff(ctx, form, [3] * 70, [3] * 65) == ([], [])                          # all rows equal
    assert check_diff(ctx, form, [3] * 70, [4] * 65) == ([64], [69])
    assert check_diff(ctx, form, [], keys) == (list(range(300)), [])                      # either side empty
    assert check_diff(ctx, form, keys, []) == ([], list(range(300)))
    assert check_diff(ctx, form, [], []) == ([], [])


@functools.lru_cache(maxsize=None)
def large_diff_case():
    n = 100003
    rng = np.random.default_rng(23)
    base = rng.integers(0, 1 << 60, size=n)
    dup = rng.integers(0, n, size=n // 50)
    base[dup] = base[(dup + 7) % n]                 # duplicates inside base
    head = base.copy()
    changed = rng.random(n) < 0.01                  # about 1 % of the rows changed
    head[changed] = rng.integers(1 << 60, 1 << 61, size=int(changed.sum()))
    head = np.concatenate([head[: n // 2], head[n // 2 + 5:], head[:40]])   # five rows dropped, forty repeated
    return base.tolist(), head.tolist()


@pytest.mark.parametrize("form", FORMS)
def test_diff_of_100003_rows_with_one_percent_changed(ctx, form):
    base, head = large_diff_case()
    added, removed = check_diff(ctx, form, base, head)
    assert 800 < len(added) < 1200 and 800 < len(removed) < 1300


# ---------------------------------------------------------------- 6. end to end
def test_compute_new_row_indices_over_two_frames(ctx, oracle_lib):
    names = ["ann", "bob", None, "dee", "bob", "eve"]
    base = {"id": column(np.array([1, 2, 3, 4, 2, 5], dtype=np.int64)), "name": column(names),
            "ok": column(np.array([True, False, True, True, False, False]))}
    # row 1 == row 4 in base (last occurrence: 4); head drops "dee", changes "eve", adds two equal rows
    head = {"id": column(np.array([1, 2, 3, 5, 6, 6], dtype=np.int64)), "name": column(["ann", "bob", None, "eva", "fay", "fay"]),
            "ok": column(np.array([True, False, True, False, True, True]))}
    want = _rowhash.compute_new_row_indices(
        _rowhash.hex_strings(_rowhash.row_hashes(list(base.values()), oracle_lib)),
        _rowhash.hex_strings(_rowhash.row_hashes(list(head.values()), oracle_lib)))
    assert want == ([3, 5], [3, 5])
    added, removed = tabular.compute_new_row_indices(base, head, ctx=ctx)
    assert (added.tolist(), removed.tolist()) == want
    assert tabular.row_hash_strings(tabular.df_hash_rows(base, ctx=ctx)) == \
        _rowhash.hex_strings(_rowhash.row_hashes(list(base.values()), oracle_lib))
    # a removed duplicate: only its last row is reported
    head2 = {k: column(v) for k, v in (("id", np.array([1], dtype=np.int64)), ("name", ["ann"]), ("ok", np.array([True])))}
    added, removed = tabular.compute_new_row_indices(base, head2, ctx=ctx)
    assert (added.tolist(), removed.tolist()) == ([], [2, 3, 4, 5])
