"""The Parquet reader's list columns on the GPU (oxh_parquet_lists_*, oxen_amd/csrc/parquet_lists.hip): pyarrow's
fixtures (tests/golden/parquet/lists_*: V1 and V2 pages of about 100 level entries, SNAPPY and ZSTD, dictionaries
that fall back to PLAIN, a 300-element row, whole pages of one RLE run) read bit for bit as tests/_parquet_lists_cases.py's
cells in both forms; a hand-cut file whose pages begin in the middle of rows; both offset widths and the widened
element words; the embedding column into cosine_similarity_device; the scratch poison; malformed level streams."""
import ctypes

import numpy as np
import pytest
import torch

import _embedding as E
import _parquet_cases as K0
import _parquet_lists_cases as K
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
NAMES = [name for name, *_ in K.LISTS] + list(K.FLAT)
DTYPE = {name: dtype for name, dtype, *_ in K.LISTS}


@pytest.fixture(scope="module")
def want():   # the fixtures' cells, computed once and left alone
    cells = K.cells(K.ROWS)
    return {**{name: K.expected(DTYPE[name], cells[name]) for name in DTYPE},
            "i": (8,) + K0.expected("i", "<i8", cells["i"]), "s": (_capi.OXH_COL_BYTES32,) + K0.expected("s", "str", cells["s"])}


def source(name, form):
    data = K0.fixture_bytes(name)
    if form == "host":
        return data
    return torch.from_numpy(np.frombuffer(b"\0" * 3 + data, dtype=np.uint8).copy()).to("cuda:0")[3:]   # the caller's bytes at an odd address


def read(ctx, name, form, **how):
    if form == "host":
        return tabular.read_parquet(source(name, form), ctx=ctx, **how)
    return tabular.read_parquet_device(source(name, form), ctx=ctx, stream=ctx.stream, **how)


def assert_list(got, want, dtype, what, wide=False):
    down = lambda t: np.asarray(t) if isinstance(t, np.ndarray) else t.cpu().numpy()   # noqa: E731
    values, offsets, validity, child = (down(t) for t in got)
    woffsets, wvalid, wchild, wvalues = want
    n, count = len(wvalid), len(wchild)
    assert offsets.dtype == (np.int64 if wide else np.int32) and np.array_equal(offsets, woffsets), what
    assert np.array_equal(K.bits(validity, n), wvalid) and not np.unpackbits(validity, bitorder="little")[n:].any(), what
    assert np.array_equal(K.bits(child, count), wchild) and not np.unpackbits(child, bitorder="little")[count:].any(), what
    assert values.dtype == np.dtype(dtype) and np.array_equal(values.view("<u%d" % values.itemsize), wvalues), what


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", K.FILES)
def test_fixtures_read_as_their_cells(ctx, want, name, form):
    got = read(ctx, name, form)
    assert list(got) == NAMES
    for col, dtype in DTYPE.items():
        assert_list(got[col], want[col], dtype, (name, col))
    for col in K.FLAT:   # the flat columns of the same file still read
        K0.assert_same(got[col], want[col], (name, col))
    cells = K.cells(K.ROWS)
    with tabular.ParquetFile(source(name, form), ctx=ctx, device=form == "device", stream=ctx.stream if form == "device" else None) as f:
        assert (f.stats.rows, f.stats.ncols, f.stats.row_groups, f.stats.unreadable_columns) == (K.ROWS, len(NAMES), 2, 0)
        native = {"<i8": _capi.OXH_CSV_INT64, "<f4": _capi.OXH_CSV_FLOAT32, "<i4": _capi.OXH_CSV_INT32, "<f8": _capi.OXH_CSV_FLOAT64}
        assert [(t.type, t.required, t.readable) for t in f.types()[:5]] == [(native[d] | _capi.OXH_PARQUET_LIST, not nl, True) for _, d, nl, _, _ in K.LISTS]
        # int64 offsets, and INT32 / FLOAT elements widened in the store
        cols, stats = f.lists([0, 1, 3], ["LargeList[Int64]", "LargeList[Float64]", "LargeList[Int64]"], with_stats=True)
        assert_list(cols[0], want["li64"], "<i8", (name, "li64 wide"), wide=True)
        widened = lambda col, to: want[col][:3] + (want[col][3].view(DTYPE[col]).astype(to).view("<u8"),)   # noqa: E731
        assert_list(cols[1], widened("lf32", "<f8"), "<f8", (name, "lf32 as Float64"), wide=True)
        assert_list(cols[2], widened("li32", "<i8"), "<i8", (name, "li32 as Int64"), wide=True)
        for s, col in zip(stats, ("li64", "lf32", "li32")):
            assert (s.null_lists, s.null_elements, s.elements) == (int((~want[col][1]).sum()), int((~want[col][2]).sum()), len(want[col][2])), (name, col)
        assert sum(c is None for c in cells["li64"]) == stats[0].null_lists > 0
        assert stats[0].pages > 2 * 3, stats   # 10 KB of 8-byte values a chunk in pages of 600 bytes (li32's indices fit one page)
        with pytest.raises(_capi.OxenError, match="column 'emb': a list column: oxh_parquet_lists_\\* read it"):
            f.columns([2], [_capi.OXH_CSV_FLOAT32])
        with pytest.raises(_capi.OxenError, match="column 'i': not a list column: oxh_parquet_columns_\\* read it"):
            f.lists([5], [_capi.OXH_PARQUET_LIST | _capi.OXH_CSV_INT64])
        with pytest.raises(_capi.OxenError, match="elements of physical type INT64 are not read as type 6"):
            f.lists([0], ["List[Int32]"])
    assert tabular.parquet_schema(K0.fixture_bytes(name), ctx=ctx)[:3] == [("li64", "List[Int64]"), ("lf32", "List[Float32]"), ("emb", "List[Float32]")]


@pytest.mark.parametrize("form", ["host", "device"])
def test_pages_that_begin_in_the_middle_of_a_row(ctx, form):
    """lists_split_rows: pyarrow begins every page with a row, so tests/golden/make_df_parquet_lists.py cuts this
    file's V1 pages itself, every 37 level entries whatever the rows do: rows run on over one and over several page
    boundaries, and pages hold no row start at all."""
    cells = K.split_cells(K.SPLIT_ROWS)
    got = read(ctx, "lists_split_rows", form)
    assert list(got) == ["v"]
    assert_list(got["v"], K.expected("<i8", cells), "<i8", form)


def test_the_embedding_column_feeds_the_similarity(ctx, want):
    got = read(ctx, "lists_v2_zstd", "device", columns=["emb", "lf32"])
    emb = tabular.embedding_from_list(got["emb"])
    assert (emb.layout, emb.dim, emb.nrows) == (_capi.OXH_EMB_FIXED, K.DIM, K.ROWS) and emb.values.data_ptr() == got["emb"].values.data_ptr()
    query = np.array([1, -2, 3, 0, -1, 2, 4, -3], np.float32)   # integers, as the cells: the sums are exact in any order
    sim = tabular.cosine_similarity_device(emb, torch.from_numpy(query).to("cuda:0"), ctx=ctx, stream=ctx.stream)
    ref = E.similarity_exact(tabular.Embedding(_capi.OXH_EMB_FIXED, K.DIM, K.ROWS, want["emb"][3].view("<f4")), query)
    assert np.array_equal(sim.sim.cpu().numpy().view(np.uint32), ref.sim.view(np.uint32)) and np.array_equal(sim.perm.cpu().numpy(), ref.perm)
    ragged = tabular.embedding_from_list(got["lf32"], dim=3)   # null lists and other lengths: the list layout over the same buffers
    assert (ragged.layout, ragged.dim) == (_capi.OXH_EMB_LIST32, 3) and ragged.offsets.data_ptr() == got["lf32"].offsets.data_ptr()
    with pytest.raises(_capi.OxenError, match="null elements inside a vector"):
        tabular.embedding_from_list(tabular.ListColumn(np.zeros(2, np.float32), np.array([0, 2], np.int32), np.array([1], np.uint8), np.array([1], np.uint8)))


def test_lists_do_not_depend_on_what_the_scratch_held(ctx, want):
    L, seen = _capi.lib(), set()
    for poison in (0x00, 0xFF, 0x5A):
        assert L.oxh_set_scratch_poison(poison) == -1
        try:
            before = L.oxh_scratch_poisoned_bytes()
            with tabular.ParquetFile(source("lists_v1_snappy", "device"), ctx=ctx, device=True, stream=ctx.stream) as f:
                cols, stats = f.lists(range(5), with_stats=True)
            assert L.oxh_scratch_poisoned_bytes() > before, "no working allocation was poisoned"
        finally:
            L.oxh_set_scratch_poison(-1)
        for col, (name, dtype, *_) in zip(cols, K.LISTS):
            assert_list(col, want[name], dtype, (name, poison))
        seen.add((tuple(stats), tuple(t.cpu().numpy().tobytes() for c in cols for t in c)))
    assert len(seen) == 1, "the lists depend on what the scratch held"


@pytest.mark.parametrize("at, byte, what", [(0, 0x01, "levels are malformed"), (5, 0x69, "levels are malformed, end early or pass the column's maximum, or a chunk does not begin with a row"),
                                            (5, 0x60, "row group 0: its pages start 501 rows, the group has 500")],
                         ids=["rep-stream-cut-short", "chunk-begins-with-rep-1", "one-row-start-too-many"])
def test_malformed_levels_are_invalid(ctx, at, byte, what):
    """Column li64's first data page of lists_v1: its repetition stream's length (26), the bit-packed run's header
    (0x33: 25 groups) and its first byte 0x68 = the levels 0 0 0 1 0 1 1 0 of rows 0 .. 3."""
    good = K0.fixture_bytes("lists_v1")
    i = good.index(bytes.fromhex("1a00000033681eed"))
    data = good[:i + at] + bytes([byte]) + good[i + at + 1:]
    with tabular.ParquetFile(data, ctx=ctx) as f:   # the file still opens and its other columns still read
        assert len(f.columns([5], [_capi.OXH_CSV_INT64])) == 1
        words = (ctypes.c_uint64 * 4)()
        col, type_word = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint32 * 1)(_capi.OXH_PARQUET_LIST | _capi.OXH_CSV_INT64)
        rc = _capi.lib().oxh_parquet_lists_host(f.handle, 1, col, type_word, None, None, None, None, None, words, words)
        assert rc == _capi.OXH_ERR_INVALID and what in _capi.lib().oxh_last_error().decode(), _capi.lib().oxh_last_error()
