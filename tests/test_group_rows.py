"""The grouping of rows by equality on key columns on the GPU (oxh_group_rows_*, oxen_amd/csrc/group_rows.hip;
oxen_amd.tabular): all five outputs of both forms -- group, count, first_idx, first_count and the four stats --
are compared for EXACT equality with the restatement of tests/_grouprows.py, a plain Python dict over tuple
keys in row order."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import _grouprows
import _rowhash
import _take
from _grouprows import BOOL, BYTES32, BYTES64, FLOAT, SIGNED, UNSIGNED, strings
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, GroupStats, RowGroups, column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "df_unique.json")
SCAN_TILE = 2048      # exclusive_scan_u32's tile (keyed_diff.hip)
GRID_CAP = 2048       # the most workgroups of a grid-stride launch
SENTINEL = 0x5A5A5A5A


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
    """(group, count, first_idx, first_count) as uint32 numpy arrays, and the stats."""
    import torch

    if form == "host":
        g = tabular.group_rows(cols, orders, ctx=ctx)
        assert all(a.dtype == np.uint32 for a in g[:4])
        return g
    dev = [device_column(c) for c in cols]
    torch.cuda.synchronize()
    g = tabular.group_rows_device(dev, orders, stream=ctx.stream, ctx=ctx)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in g[:4])
    return RowGroups(*(t.cpu().numpy().view(np.uint32) for t in g[:4]), g.stats)


def same(got, want, who):
    for name in ("group", "count", "first_idx", "first_count"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape, (who, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError((who, name, "first difference at", at, g[at:at + 4].tolist(), w[at:at + 4].tolist()))
    assert tuple(got.stats) == tuple(want.stats), (who, got.stats, want.stats)


def check(ctx, cols, orders=None, forms=FORMS):
    """Both forms against the restatement; returns the restatement."""
    cols = [c if isinstance(c, Column) else column(c) for c in cols]
    orders = [SIGNED] * len(cols) if orders is None else list(orders)
    want = _grouprows.group_rows(cols, orders)
    for form in forms:
        same(run(ctx, form, cols, orders), want, form)
    return want


def with_nulls(c, rng, bit=5):
    """A third of the rows null, the validity bitmap's row 0 at `bit`."""
    return c._replace(validity=_rowhash.packed_at(rng.random(c.nrows) > 1 / 3, bit), validity_bit=bit)


# ---------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 9 * SCAN_TILE + 1, 2**19 + 3])
def test_sizes(ctx, n):
    """Around a wave, around the scan's tile, ten tiles -- where the tile sums outgrow one tile --, and past the
    2 048-workgroup cap of the grid-stride kernels. Int64 keys from about n / 3 values; all distinct; all equal
    (one atomic address, largest == n)."""
    assert 2**19 + 3 > GRID_CAP * 256
    rng = np.random.default_rng(n)
    few = rng.integers(-2**62, 2**62, size=max(1, n // 3))[rng.integers(0, max(1, n // 3), size=n)].astype(np.int64)
    want = check(ctx, [few])
    assert want.stats[0] <= max(1, n // 3)
    distinct = (rng.permutation(n).astype(np.int64) << 20) - 7
    assert check(ctx, [distinct]).stats == (n, 0, 1, 0)
    equal = np.full(n, -0x0123456789ABCDEF, dtype=np.int64)
    assert check(ctx, [equal]).stats == (1, n if n > 1 else 0, n, 0)
    if n > GRID_CAP * 256:   # the invariants that need no oracle
        import torch

        dev = [device_column(column(few))]
        torch.cuda.synchronize()
        g = tabular.group_rows_device(dev, stream=ctx.stream, ctx=ctx)
        group, first_idx, first_count = (t.cpu().numpy().view(np.uint32).astype(np.int64) for t in (g.group, g.first_idx, g.first_count))
        assert (group <= np.arange(n)).all() and np.array_equal(group[group], group)
        assert np.array_equal(first_idx, np.nonzero(group == np.arange(n))[0]) and int(first_count.sum()) == n


# ---------------------------------------------------------------- 2. delimiting
def test_cells_are_delimited_where_the_row_hash_collides(ctx):
    """Each pair has ONE row hash (undelimited cells, a null without bytes) and must land in two groups."""
    i64 = lambda values, valid: column(np.array(values, dtype=np.int64), validity=valid)  # noqa: E731
    pairs = {
        "ab|c vs a|bc": [column(["ab", "a"]), column(["c", "bc"])],
        "null,5 vs 5,null": [i64([0, 5], [False, True]), i64([5, 0], [True, False])],
        "null vs empty": [column([None, ""])],
        "null vs 0": [i64([0, 0], [False, True])],
        "null vs false": [Column(BOOL, 2, np.array([0b00], dtype=np.uint8), None, np.array([0b10], dtype=np.uint8))],
        "int8 1 then empty vs null then 01": [column(np.array([1, 0], dtype=np.int8), validity=[True, False]), column(["", "\x01"])],
    }
    collide = 0
    for name, cols in pairs.items():
        want = check(ctx, cols)
        assert want.stats == (2, 0, 1, 0) and want.group.tolist() == [0, 1], name
        h = tabular.row_hashes(cols, ctx=ctx)
        collide += bool((h[0] == h[1]).all())
    assert collide >= 3      # ab|c, null,5 and null vs empty at the least: why the key image exists
    h = tabular.row_hashes(pairs["ab|c vs a|bc"], ctx=ctx)
    assert (h[0] == h[1]).all()
    # all of them in one frame, each row twice: six pairs of groups of two
    a = strings([b"ab", b"a", b"", b"", b"x", b"x"] * 2, valid=[True, True, False, True, True, True] * 2, bit=3)
    b = column(np.array([0, 0, 0, 0, 0, 5] * 2, dtype=np.int64), validity=[True, True, True, True, False, True] * 2)
    c = strings([b"c", b"bc", b"", b"", b"", b""] * 2, kind=BYTES64)
    assert check(ctx, [a, b, c]).stats == (6, 12, 2, 0)


# ---------------------------------------------------------------- 3. floats
NAN64 = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                  0xFFF5A5A5A5A5A5A5], dtype=np.uint64)
NAN32 = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFA55AA5], dtype=np.uint32)


@pytest.mark.parametrize("width", [4, 8])
def test_floats(ctx, width):
    """+-0.0 are one group and the NaNs of every sign and payload another under OXH_SORT_FLOAT, and as many groups
    as bit patterns under OXH_SORT_UNSIGNED; +-inf and the denormals stay distinct under both."""
    ft, ut, nans = (np.float32, np.uint32, NAN32) if width == 4 else (np.float64, np.uint64, NAN64)
    tiny = np.finfo(ft).smallest_subnormal
    plain = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 2 * tiny, np.finfo(ft).tiny, 1.0, -1.0, 0.0, -0.0], dtype=ft)
    values = np.concatenate([plain.view(ut), nans, nans[::-1]]).view(ft)
    rng = np.random.default_rng(width)
    values = values[rng.permutation(values.size)]
    assert np.array_equal(np.sort(values.view(ut)), np.sort(np.concatenate([plain.view(ut), nans, nans])))   # the payloads stay
    c = Column(width, values.size, values)
    want = check(ctx, [c], [FLOAT])
    assert want.stats == (2 + 8, 4 + 12, 12, 0)          # zeros, NaNs, and eight values of their own
    want = check(ctx, [c], [UNSIGNED])
    assert want.stats == (2 + 8 + 6, 4 + 12, 2, 0)        # +0.0 and -0.0 apart, six NaN patterns, each twice
    check(ctx, [c], [SIGNED])
    big = np.concatenate([values, rng.standard_normal(SCAN_TILE).astype(ft)])[rng.permutation(values.size + SCAN_TILE)]
    check(ctx, [with_nulls(Column(width, big.size, big), rng)], [FLOAT])


# ---------------------------------------------------------------- 4. every kind, sliced
@functools.lru_cache(maxsize=None)
def mixed_frame():
    """Every OXH_COL_* kind, a third of the rows null in each column, validity bitmaps and the boolean values
    starting at bit offsets that are no multiple of 8, offsets[0] != 0, null byte cells with bytes underneath;
    few values per column, so that rows repeat."""
    n = SCAN_TILE + 333
    rng = np.random.default_rng(44)
    words = [b"", b"a", b"ab", b"abc", b"a\0", b"\xff\xfe", b"longer than eight bytes"]
    frame = {
        "i8": with_nulls(column(rng.integers(-1, 2, size=n).astype(np.int8)), rng, bit=1),
        "f32": with_nulls(column(rng.choice(np.array([0.0, -0.0, 1.5, np.nan], dtype=np.float32), size=n)), rng, bit=3),
        "i64": with_nulls(column(rng.integers(0, 2, size=n).astype(np.int64) << 40), rng, bit=5),
        "b": with_nulls(Column(BOOL, n, _rowhash.packed_at(rng.random(n) < 0.5, 13), None, None, 13, 0), rng, bit=7),
        "s": strings([words[k] for k in rng.integers(0, len(words), size=n)], BYTES32, rng.random(n) > 1 / 3, 5, lead=b"LEAD!"),
        "ls": strings([words[k] for k in rng.integers(0, 3, size=n)], BYTES64, rng.random(n) > 1 / 3, 2, lead=b"xy"),
    }
    assert frame["s"].offsets[0] == 5 and frame["ls"].offsets[0] == 2 and frame["b"].value_bit == 13
    return frame


MIXED_ORDERS = {"i8": SIGNED, "f32": FLOAT, "i64": SIGNED, "b": SIGNED, "s": SIGNED, "ls": SIGNED}


@pytest.mark.parametrize("names", [["i8"], ["f32"], ["i64"], ["b"], ["s"], ["ls"], ["i8", "f32", "i64", "b", "s", "ls"], ["ls", "b", "i8"]])
def test_every_kind_sliced(ctx, names):
    frame = mixed_frame()
    want = check(ctx, [frame[x] for x in names], [MIXED_ORDERS[x] for x in names])
    assert want.stats[1] > 0 and want.stats[0] > 1
    if len(names) == 6:
        assert 100 < want.stats[0] < frame["i8"].nrows


# ---------------------------------------------------------------- 5. the short / long boundary
def test_short_long_boundary(ctx):
    """String keys whose ENCODED image (tag + 4 bytes of length + the cell, behind an Int8 cell of tag + 1) is
    239, 240, 241 B and about 2 KiB, each with a duplicate and a near-duplicate that differs in the last byte,
    among short rows, in one call."""
    rng = np.random.default_rng(5)
    cells, small = [], []
    for image in (239, 240, 241, 2048):
        body = bytes(rng.integers(0, 256, size=image - 7 - 1, dtype=np.uint8))
        cells += [body + b"\x01", body + b"\x01", body + b"\x02"]
    shorts = [bytes(rng.integers(97, 100, size=int(l), dtype=np.uint8)) for l in rng.integers(0, 4, size=500)]
    cells = shorts[:250] + cells + shorts[250:] + cells[::-1]
    tag = column(np.zeros(len(cells), dtype=np.int8))
    cols = [tag, strings(cells)]
    keys = _grouprows.row_keys(cols)
    assert sorted({_grouprows.encoded_length(cols, k) for k in keys if len(k[1]) > 100}) == [239, 240, 241, 2048]
    want = check(ctx, cols)
    assert want.stats[3] == 2 * 2 * 3 and want.stats[2] >= 4    # the 241-B and the 2-KiB images, both copies
    # int64 offsets: the length prefix is 8 bytes, so every image above is 4 B longer and all four sizes are long
    want64 = check(ctx, [tag, strings(cells, BYTES64)])
    assert want64.stats[3] == 2 * 4 * 3 and want64.stats[:3] == want.stats[:3]
    # long rows only
    only = [c for c in cells if len(c) > 1000]
    assert check(ctx, [strings(only)]).stats == (2, 6, 4, 6)


# ---------------------------------------------------------------- 6. low cardinality
@pytest.mark.parametrize("labels", [3, 100])
def test_low_cardinality_labels(ctx, labels):
    """The `--unique_count label` shape: 2^18 rows over a few labels of one string column. first_count exact."""
    n = 2**18
    rng = np.random.default_rng(labels)
    names = [b"label-%03d" % k for k in range(labels)]
    pick = rng.integers(0, labels, size=n)
    col = strings([names[k] for k in pick.tolist()])
    want = check(ctx, [col], forms=["device"])
    assert want.stats[0] == labels and int(want.first_count.sum()) == n
    counts = np.bincount(pick, minlength=labels)
    order = [int(pick[i]) for i in want.first_idx.tolist()]
    assert want.first_count.tolist() == counts[order].tolist()
    if labels == 3:
        same(run(ctx, "host", [col], [SIGNED]), want, "host")


# ---------------------------------------------------------------- 7. cross-check with the sort, on the device
def test_duplicated_equals_the_sort_s_tied_rows(ctx):
    """stats.duplicated against the sort's stats3[2] -- "rows that equal another row on every key", reached
    through radix passes, not through a hash -- and group[perm] constant exactly on the sort's runs of equal rows."""
    import torch

    n = 2**16
    rng = np.random.default_rng(7)
    cols = [with_nulls(column(rng.integers(0, 40, size=n).astype(np.int32)), rng),
            column(np.round(rng.standard_normal(n), 1)),
            strings([bytes(rng.integers(97, 99, size=int(l), dtype=np.uint8)) for l in rng.integers(0, 3, size=n)])]
    orders = [SIGNED, FLOAT, SIGNED]
    dev = [device_column(c) for c in cols]
    torch.cuda.synchronize()
    g = tabular.group_rows_device(dev, orders, stream=ctx.stream, ctx=ctx)
    perm, stats = tabular.sort_indices_device(dev, orders, stream=ctx.stream, ctx=ctx)
    assert g.stats.duplicated == stats.tied and 0 < stats.tied < n
    group = g.group.cpu().numpy().view(np.uint32)[perm.cpu().numpy().view(np.uint32)]
    boundaries = int((np.diff(group.astype(np.int64)) != 0).sum()) + 1
    assert boundaries == g.stats.groups      # every group is one run of the sorted order, and no two runs share one
    assert np.unique(group).size == g.stats.groups


# ---------------------------------------------------------------- 8. NULL outputs in every combination
def test_null_outputs_in_every_combination(ctx):
    """The arrays not asked for are not written (there is nothing to write to); those asked for are the
    restatement's, and first_idx / first_count from `groups` on keep their sentinel."""
    import torch

    n = 700
    rng = np.random.default_rng(8)
    cols = [column(rng.integers(0, 90, size=n).astype(np.int64))]
    want = _grouprows.group_rows(cols)
    groups = want.stats[0]
    expect = [want.group, want.count, np.concatenate([want.first_idx, np.full(n - groups, SENTINEL, np.uint32)]),
              np.concatenate([want.first_count, np.full(n - groups, SENTINEL, np.uint32)])]
    dev = device_column(cols[0])
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    tables = tabular._tables([dev], ptr)
    host_keep = []
    host_tables = tabular._tables(cols, lambda a: None if a is None else host_keep.append(np.ascontiguousarray(a)) or host_keep[-1].ctypes.data)
    for mask in range(16):
        outs = [torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(4)]
        stats = np.full(4, 7, dtype=np.uint64)
        torch.cuda.synchronize()
        rc = _capi.lib().oxh_group_rows_device(ctx.handle, n, 1, *tables, (ctypes.c_uint32 * 1)(0),
                                               *[None if mask >> k & 1 else o.data_ptr() for k, o in enumerate(outs)],
                                               stats.ctypes.data_as(_capi._u64p), ctx.stream)
        assert rc == _capi.OXH_OK and tuple(stats.tolist()) == want.stats, mask
        for k, o in enumerate(outs):
            got = o.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, np.full(n, SENTINEL, np.uint32) if mask >> k & 1 else expect[k]), (mask, k)
        houts = [np.full(n, SENTINEL, dtype=np.uint32) for _ in range(4)]
        rc = _capi.lib().oxh_group_rows_host(ctx.handle, n, 1, *host_tables, (ctypes.c_uint32 * 1)(0),
                                             *[None if mask >> k & 1 else o.ctypes.data for k, o in enumerate(houts)],
                                             stats.ctypes.data_as(_capi._u64p))
        assert rc == _capi.OXH_OK and tuple(stats.tolist()) == want.stats, mask
        for k, o in enumerate(houts):
            assert np.array_equal(o, np.full(n, SENTINEL, np.uint32) if mask >> k & 1 else expect[k]), ("host", mask, k)


# ---------------------------------------------------------------- 9. what the device refuses
def test_decreasing_offsets_on_the_device_form(ctx):
    """A decreasing pair of offsets is a cell of length 0 and OXH_ERR_INVALID: the defined error path of every
    tabular entry. Nothing outside a named span is read; the outputs are those of the frame with that cell
    empty; the next call is fine."""
    import torch

    good = column(["ab", "cd", "", "g", "", "ab"])
    broken = good._replace(offsets=np.array([0, 2, 4, 3, 5, 5, 7], dtype=np.int32))   # a decreasing pair at row 2
    other = column(np.array([1, 1, 2, 1, 2, 1], dtype=np.int8))
    want = _grouprows.group_rows([other, broken], empty={1: {2}})
    assert want.group.tolist() == [0, 1, 2, 3, 2, 0]
    dev = [device_column(other), device_column(broken)]
    outs = [torch.full((6,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(4)]
    stats = np.full(4, 7, dtype=np.uint64)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    rc = _capi.lib().oxh_group_rows_device(ctx.handle, 6, 2, *tabular._tables(dev, ptr), (ctypes.c_uint32 * 2)(0, 0),
                                           *[o.data_ptr() for o in outs], stats.ctypes.data_as(_capi._u64p), ctx.stream)
    assert rc == _capi.OXH_ERR_INVALID and b"offsets" in _capi.lib().oxh_last_error()
    got = [o.cpu().numpy().view(np.uint32) for o in outs]
    groups = want.stats[0]
    assert np.array_equal(got[0], want.group) and np.array_equal(got[1], want.count)
    assert np.array_equal(got[2][:groups], want.first_idx) and np.array_equal(got[3][:groups], want.first_count)
    assert (got[2][groups:] == SENTINEL).all() and tuple(stats.tolist()) == want.stats
    with pytest.raises(_capi.OxenError, match="decrease"):
        tabular.group_rows([other, broken], ctx=ctx)                # the host form reads the offsets itself
    check(ctx, [other, good])                                        # and the next call is fine


# ---------------------------------------------------------------- 10. compositions
def golden_frame(case, dtypes, which="frame"):
    numpy_of = {"f64": np.float64, "bool": bool}
    out = {}
    for name, values in case[which].items():
        dt = dtypes[name]
        if dt == "str":
            out[name] = column(values)
        elif dt == "u32":
            out[name] = Column(4, len(values), np.array(values, dtype=np.uint32))
        else:
            out[name] = column(np.array(values, dtype=numpy_of[dt]))
    return out


def test_unique_and_unique_count_reproduce_the_reference_s_frames(ctx):
    """`unique` / `unique_count` then `sort_by`: the three expected frames of tabular.rs:1803-1901."""
    fx = json.load(open(GOLDEN))
    for case in fx["cases"]:
        frame = golden_frame(case, fx["dtypes"])
        op = tabular.unique if case["op"] == "unique" else tabular.unique_count
        got = tabular.sort_by(op(frame, case["fields"], ctx=ctx), case["sort_by"], ctx=ctx)
        want = golden_frame(case, fx["dtypes"], "expected")
        assert list(got) == list(want), case["name"]
        for name, c in want.items():
            assert got[name].kind == c.kind and _take.pylist(got[name]) == _take.pylist(c), (case["name"], name)
        want_groups = _grouprows.group_rows([frame[x] for x in case["fields"]])
        assert tabular.is_duplicated(frame, case["fields"], ctx=ctx).tolist() == (want_groups.count > 1).tolist()
        assert tabular.n_duped_rows(frame, case["fields"], ctx=ctx) == want_groups.stats[1]
    count = tabular.unique_count(golden_frame(fx["cases"][2], fx["dtypes"]), "label", ctx=ctx)["count"]
    assert count.kind == _capi.OXH_COL_FIXED4 and count.values.dtype == np.uint32 and count.values.tolist() == [3, 1]


def test_is_duplicated_and_n_duped_rows_on_the_mixed_frame(ctx):
    frame = mixed_frame()
    names = ["i8", "f32", "s"]
    orders = {x: MIXED_ORDERS[x] for x in names}
    want = _grouprows.group_rows([frame[x] for x in names], [orders[x] for x in names])
    assert tabular.is_duplicated(frame, names, ctx=ctx, orders=orders).tolist() == (want.count > 1).tolist()
    assert tabular.n_duped_rows(frame, names, ctx=ctx, orders=orders) == want.stats[1]
    u = tabular.unique(frame, names, ctx=ctx, orders=orders)
    taken = _take.take(list(frame.values()), want.first_idx)
    assert list(u) == list(frame)
    for got, t in zip(u.values(), taken):
        assert _take.pylist(got, text=False) == _take.pylist(t, text=False)


def test_unique_count_over_an_arrow_table(ctx):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(10)
    n = 400
    table = pa.table({
        "label": pa.array([["dog", "cat", "unknown", ""][k] for k in rng.integers(0, 4, size=n)], type=pa.string(),
                          mask=rng.random(n) < 0.2),
        "score": pa.array(rng.choice([0.0, -0.0, 1.0, float("nan")], size=n).tolist(), type=pa.float64()),
        "flag": pa.array((rng.random(n) < 0.5).tolist(), type=pa.bool_(), mask=rng.random(n) < 0.2),
    }).slice(3)
    frame = tabular.columns_from_arrow(table)
    names = ["label", "score", "flag"]
    orders = tabular.sort_orders_from_arrow(table.schema, names)
    want = _grouprows.group_rows([frame[x] for x in names], orders)
    got = tabular.unique_count(frame, names, ctx=ctx, orders=orders)
    assert got["count"].values.tolist() == want.first_count.tolist()
    for name, t in zip(names, _take.take([frame[x] for x in names], want.first_idx)):
        assert _take.pylist(got[name], text=False) == _take.pylist(t, text=False), name
