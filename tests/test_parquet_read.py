"""The Parquet reader on the GPU (oxh_parquet_*, oxen_amd/csrc/parquet_read.hip): what `write_parquet*` wrote reads
back to the frame bit for bit in both forms; pyarrow's fixtures (tests/golden/parquet: V1 and V2 pages, dictionaries
that fall back to PLAIN, RLE booleans, 100-row pages that share validity bytes) read as tests/_parquet_cases.py's
cells, and as pyarrow reads them where it imports; selections, widenings and a file past one capped launch."""
import io

import numpy as np
import pytest
import torch

import _csvwrite_call as C
import _parquet_cases as K
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
W = C.W
NAMES = [name for name, _, _ in K.COLUMNS]
fixture_bytes, to_host, parts, assert_same = K.fixture_bytes, K.to_host, K.parts, K.assert_same


def edge_frame(n):   # every column type under every validity shape, at n rows, with bit offsets the file forgets
    alt = lambda cells: [None if r % 2 else c for r, c in enumerate(cells)]  # noqa: E731
    edges = {63, 64, 1023, 1024, 127, 128}
    ints = [[-(1 << 63), (1 << 63) - 1, 0, -1, r][r % 5] for r in range(n)]
    floats = [[0.5, -0.0, float("nan"), 0.0, float("inf"), float("-inf"), -2.5e300][r % 7] for r in range(n)]
    bools = [r % 3 == 0 for r in range(n)]
    strings = [b"x" * [0, 1, 15, 16, 17][r % 5] + b"\xff" * (r % 2) for r in range(n)]
    if n > 600:
        strings[600] = b"a long cell " * 60   # a whole wave's copy
    spec = [("i_plain", W.INT64, ints, {}), ("i_alt", W.INT64, alt(ints), dict(nbit=1)),
            ("i_edges", W.INT64, [None if r in edges else v for r, v in enumerate(ints)], {}), ("i_allnull", W.INT64, [None] * n, {}),
            ("f_mixed", W.FLOAT64, [None if r % 9 == 4 else v for r, v in enumerate(floats)], dict(nbit=7)),
            ("b_plain", W.BOOL, bools, dict(vbit=1)), ("b_alt", W.BOOL, alt(bools), dict(vbit=7, nbit=1)),
            ("b_edges", W.BOOL, [None if r in edges or r % 10 == 9 else v for r, v in enumerate(bools)], dict(nbit=7)),
            ("s_plain", W.STRING, strings, dict(lead=b"lead")), ("s_alt", W.STRING64, alt(strings), dict(nbit=1)),
            ("s_edges", W.STRING, [None if r in edges else v for r, v in enumerate(strings)], {})]
    return {name: C.host_column(t, cells, **kw) for name, t, cells, kw in spec}, [t for _, t, _, _ in spec]


@pytest.mark.parametrize("cut", [{}, dict(rows_per_group=1024, page_bytes=4096)], ids=["default", "g1024"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_round_trip_of_both_forms(ctx, n, cut):
    frame, types = edge_frame(n)
    schema = {name: ("LargeString" if t == W.STRING64 else None) for name, t in zip(frame, types)}
    data = tabular.write_parquet(frame, types=types, ctx=ctx, **cut)
    d_data = tabular.write_parquet_device({k: C.to_device(c) for k, c in frame.items()}, types=types, ctx=ctx, stream=ctx.stream, **cut)
    assert tabular.parquet_shape(data, ctx=ctx) == (len(frame), n)
    for got in (tabular.read_parquet(data, schema=schema, ctx=ctx), tabular.read_parquet_device(d_data, schema=schema, ctx=ctx, stream=ctx.stream)):
        assert list(got) == list(frame)
        for name in frame:
            assert_same(got[name], frame[name], (name, n))


@pytest.fixture(scope="module")
def want():   # the fixtures' cells, computed once and left alone
    return K.wanted(K.COLUMNS, K.cells(K.ROWS))


def read_fixture(ctx, name, form, **how):
    data = fixture_bytes(name)
    if form == "host":
        return tabular.read_parquet(data, ctx=ctx, **how)
    d_data = torch.from_numpy(np.frombuffer(b"\0" * 3 + data, dtype=np.uint8).copy()).to("cuda:0")[3:]   # the caller's bytes at an odd address
    return tabular.read_parquet_device(d_data, ctx=ctx, stream=ctx.stream, **how)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", K.FILES)
def test_fixtures_read_as_their_cells(ctx, want, name, form):
    got = read_fixture(ctx, name, form)
    assert list(got) == NAMES
    for col in NAMES:
        assert_same(got[col], want[col], (name, col))
    with tabular.ParquetFile(fixture_bytes(name), ctx=ctx) as f:
        assert (f.stats.rows, f.stats.ncols, f.stats.row_groups, f.stats.unreadable_columns) == (K.ROWS, len(NAMES), 2, 0)
        assert (f.stats.dict_pages > 0) == ("dict" in name) and f.stats.data_pages > 2 * len(NAMES)   # a chunk of 4 000 B cut at 600 has several
        assert [t.required for t in f.types()] == [r for _, _, r in K.COLUMNS] and all(t.readable for t in f.types())
        _, stats = f.measure(range(len(NAMES)), [t.type for t in f.types()])
        assert [s.nulls for s in stats] == [int((~want[c][1]).sum()) for c in NAMES]
        assert (stats[0].dict_values > 0) == ("dict" in name) and stats[5].value_bytes == int(want["s"][3][-1])
    try:   # a second opinion where pyarrow imports
        import pyarrow.parquet as pq
    except ImportError:
        return
    table = pq.read_table(io.BytesIO(fixture_bytes(name)))
    for col, dtype, _ in K.COLUMNS:
        theirs = table.column(col).to_pylist()
        assert_same(got[col], (want[col][0],) + K.expected(col, dtype, theirs), (name, col, "pyarrow"))


def test_selection_and_widening(ctx, want):
    picked = ["u", "f64", "i32", "f32", "s"]
    got = read_fixture(ctx, "v2_dict_fallback", "device", columns=picked, schema={"i32": "Int64", "f32": "Float64", "s": "LargeString"})
    assert list(got) == picked
    cells = K.cells(K.ROWS)
    i32 = np.array([0 if c is None else c for c in cells["i32"]], dtype="<i4")
    assert_same(got["i32"], (8, want["i32"][1], i32.astype("<i8").view("<u8"), None), "i32 as Int64")
    assert_same(got["f32"], (8, want["f32"][1], np.array(cells["f32"], dtype="<f4").astype("<f8").view("<u8"), None), "f32 as Float64")
    assert_same(got["s"], (_capi.OXH_COL_BYTES64,) + want["s"][1:], "s as LargeString")
    assert got["s"].offsets.dtype == torch.int64
    for col in ("u", "f64"):
        assert_same(got[col], want[col], col)
    again = read_fixture(ctx, "v1_dict_fallback", "host", columns=[8, 7, 6, 5, 4, 3, 2, 1, 0])
    assert list(again) == NAMES[::-1] and all(np.array_equal(parts(again[c])[2], parts(to_host(read_fixture(ctx, "v2_plain", "host")[c]))[2]) for c in NAMES)
    with pytest.raises(_capi.OxenError, match="physical type INT64 is not read as type 6"):
        read_fixture(ctx, "v2_plain", "host", columns=["i64"], schema={"i64": "Int32"})


def test_an_unsupported_column_does_not_stop_the_others(ctx):
    data, cells = fixture_bytes("unsupported"), K.unsupported_cells(K.UNSUPPORTED_ROWS)
    with tabular.ParquetFile(data, ctx=ctx) as f:
        assert f.stats.unreadable_columns == 1 and [t.readable for t in f.types()] == [True, False, True]
        assert tabular.parquet_schema(data, ctx=ctx) == [("a", "Int64"), ("fixed", None), ("d", "Int32")]
    got = tabular.read_parquet(data, columns=["d", "a"], ctx=ctx)   # a DATE is its int32 days
    valid = np.array([c is not None for c in cells["a"]])
    assert_same(got["a"], (8, valid, np.array([c or 0 for c in cells["a"]], dtype="<i8").view("<u8"), None), "a")
    assert_same(got["d"], (4, valid, np.array([c or 0 for c in cells["d"]], dtype="<i4").view("<u4"), None), "d")
    with pytest.raises(_capi.OxenError, match="column 'fixed': FIXED_LEN_BYTE_ARRAY is not read"):
        tabular.read_parquet(data, ctx=ctx)


@pytest.mark.parametrize("form", ["host", "device"])
def test_more_pages_than_one_launch(ctx, form):
    """600 dictionary-coded V2 pages a column, more than the page kernels' 512 waves: the second round of the levels,
    the indices and the dictionary chase, whose counts go on adding up."""
    cells = K.many_cells(K.MANY_ROWS)
    want = K.wanted(K.MANY_COLUMNS, cells)
    got = read_fixture(ctx, "many_pages", form)
    for name, _, _ in K.MANY_COLUMNS:
        assert_same(got[name], want[name], name)
    with tabular.ParquetFile(fixture_bytes("many_pages"), ctx=ctx) as f:
        _, stats = f.measure(range(3), [t.type for t in f.types()])
    assert all(s.pages > 512 for s in stats), stats
    nulls = [int((~want[name][1]).sum()) for name, _, _ in K.MANY_COLUMNS]
    assert [s.nulls for s in stats] == nulls and [s.dict_values for s in stats[:2]] == [K.MANY_ROWS - k for k in nulls[:2]]


def test_more_rows_than_one_launch(ctx):
    """600 000 rows in 4 KiB pages: more rows than a capped grid has lanes (2 048 x 256), so the row kernels' second
    round runs, and 586 PLAIN pages a column, more than the page kernels' 512 waves."""
    n = 600000
    rng = np.random.default_rng(11)
    pack = lambda mask: np.packbits(mask, bitorder="little")  # noqa: E731
    valid = [rng.random(n) >= 0.1 for _ in range(3)]
    lens = np.where(valid[2], rng.integers(0, 14, n), 0)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    frame = {"i": tabular.Column(8, n, rng.integers(-1 << 62, 1 << 62, n), None, pack(valid[0])),
             "b": tabular.Column(_capi.OXH_COL_BOOL, n, pack(rng.random(n) < 0.5), None, pack(valid[1])),
             "s": tabular.Column(_capi.OXH_COL_BYTES32, n, rng.integers(97, 123, int(offsets[-1])).astype(np.uint8), offsets, pack(valid[2]))}
    d_data = tabular.write_parquet_device({k: C.to_device(c) for k, c in frame.items()}, types=[W.INT64, W.BOOL, W.STRING], page_bytes=4096,
                                          ctx=ctx, stream=ctx.stream)
    got = tabular.read_parquet_device(d_data, ctx=ctx, stream=ctx.stream)
    for name in frame:
        assert_same(got[name], frame[name], name)
