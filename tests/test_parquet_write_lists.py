"""The Parquet writer's LIST columns on the GPU (oxh_write_parquet_lists_*, oxen_amd/csrc/parquet_write_lists.hip):
`write_parquet` and `write_parquet_device` give identical bytes, and `pyarrow.parquet.read_table` reads them back to the
frame cell for cell -- list validity, lengths, element validity, element bits -- as does this library's own
`read_parquet`. The shapes are the smallest that reach every path: wave, tile and page edges in rows and in entries,
both forms of both level streams, the straight copy and the ranked values, the 4 096-entry block and the launch caps."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import _csvwrite_call as C
import test_parquet_write as T
from oxen_amd import _capi, tabular
from oxen_amd.tabular import _ListCells

pytestmark = pytest.mark.gpu
W = C.W


def bits_of(bitmap, at, count=None):   # the bits of an LSB-first bitmap at the positions `at` (or at .. at + count)
    every = np.unpackbits(np.asarray(bitmap, dtype=np.uint8), bitorder="little").astype(bool)
    return every[at:at + count] if count is not None else every[at]


def lists(dtype, lens, null_list=None, null_elem=None, wide=False, first=0, vbit=0, cbit=0):
    """A host list column of rows of `lens` elements: null_list(r) / null_elem(e) mark the nulls over the rows / over the
    elements array; offsets[0] = first; vbit / cbit: the bit offsets of the two bitmaps."""
    lens = np.asarray(lens, dtype=np.int64)
    offsets = np.concatenate([[first], first + np.cumsum(lens)]).astype(np.int64 if wide else np.int32)
    count = int(offsets[-1])
    values = (np.arange(count) * 7 - 1000).astype(dtype) if np.dtype(dtype).kind == "i" else (np.arange(count) / 8 - 3).astype(dtype)
    packed = lambda mask, bit0: np.packbits(np.concatenate([np.ones(bit0, dtype=bool), mask]), bitorder="little")   # noqa: E731
    validity = None if null_list is None else packed(~null_list(np.arange(len(lens))), vbit)
    child = None if null_elem is None else packed(~null_elem(np.arange(count)), cbit)
    return _ListCells(np.dtype(dtype).itemsize, len(lens), values, offsets, validity, 0, vbit, child, cbit)


def cells_of(c):
    """(list validity, lengths with a null list's 0, the written elements' validity, the valid elements' bits)."""
    offsets = np.asarray(c.offsets, dtype=np.int64)
    valid = np.ones(c.nrows, dtype=bool) if c.validity is None else bits_of(c.validity, c.validity_bit, c.nrows)
    lens = np.where(valid, np.diff(offsets), 0)
    at = np.repeat(offsets[:-1] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))   # elements under a null list are not written
    present = np.ones(len(at), dtype=bool) if c.child_validity is None or not len(at) else bits_of(c.child_validity, c.child_bit + at)
    return valid, lens, present, np.asarray(c.values).view(f"<u{c.kind}")[at][present]


def arrow_cells(col):
    col = col.combine_chunks()
    flat = col.flatten()
    width = flat.type.bit_width // 8
    return (~np.asarray(col.is_null()), np.asarray(col.value_lengths().fill_null(0)), ~np.asarray(flat.is_null()),
            flat.drop_null().to_numpy(zero_copy_only=False).view(f"<u{width}"))


def check(data, frame, stats):
    table, back = pq.read_table(io.BytesIO(data)), tabular.read_parquet(data)
    assert table.column_names == list(frame) == list(back)
    nulls = 0
    for name, c in frame.items():
        col = table.column(name)
        if not isinstance(c, _ListCells):
            valid, values = T.cells_of(c)
            got = col.combine_chunks().drop_null()
            assert np.array_equal(~np.asarray(col.combine_chunks().is_null()), valid), name
            assert got.cast(pa.binary()).to_pylist() == values if isinstance(values, list) else np.array_equal(got.to_numpy().view("<u8"), values), name
        else:
            b, want = back[name], cells_of(c)
            valid = want[0]
            assert col.type == pa.list_(pa.field("element", pa.from_numpy_dtype(c.values.dtype))), (name, col.type)
            for reader, got in (("pyarrow", arrow_cells(col)), ("read_parquet", cells_of(_ListCells(c.kind, c.nrows, b.values, b.offsets, b.validity, 0, 0, b.child_validity)))):
                for part, g, w in zip(("list validity", "lengths", "element validity", "element bits"), got, want):
                    assert np.array_equal(g, w), (name, reader, part)
        nulls += int((~valid).sum())
    assert stats.bytes == len(data) and stats.nulls == nulls, stats   # null lists and null cells; null elements are not counted


def to_device(c):
    if not isinstance(c, _ListCells):
        return C.to_device(c)
    return c._replace(**{f: torch.from_numpy(np.ascontiguousarray(getattr(c, f))).to("cuda:0") for f in ("values", "offsets", "validity", "child_validity")
                         if getattr(c, f) is not None})


def both_forms(ctx, frame, **how):
    host, stats = tabular.write_parquet(frame, ctx=ctx, with_stats=True, **how)
    dev, dstats = tabular.write_parquet_device({n: to_device(c) for n, c in frame.items()}, ctx=ctx, stream=ctx.stream, with_stats=True, **how)
    assert dev.cpu().numpy().tobytes() == host and dstats == stats
    check(host, frame, stats)
    return pq.ParquetFile(io.BytesIO(host)).metadata


def edge_frame(n):
    r = np.arange(n)
    return {
        "emb": lists("float32", np.full(n, 3)),                                               # both streams RLE, the straight copy
        "tok": lists("int64", r % 5, lambda r: r % 7 == 3, lambda e: e % 4 == 1, wide=True),
        # two elements a row, so entry == element: nulls at entries 63, 64, 4 095 and 4 096 of a default page and of a one-tile page
        "box": lists("float64", np.full(n, 2), lambda r: r < 0, lambda e: np.isin(e % 2048, (63, 64)) | np.isin(e, (4095, 4096)), vbit=1, cbit=7),
        "flag": lists("int32", r % 2, lambda r: r % 5 == 0),                                   # an entry a row: repetition is RLE
        "cut": lists("int32", np.full(n, 2), lambda r: r % 3 == 1, first=5),                   # offsets[0] != 0; the null lists span elements
        "id": C.host_column(W.INT64, [None if k % 11 == 2 else k * 3 for k in range(n)]),
        "s": C.host_column(W.STRING, [None if k % 13 == 5 else b"x" * (k % 9) for k in range(n)]),
    }


@pytest.mark.parametrize("cut", [{}, dict(rows_per_group=1024, page_bytes=4096)], ids=["default", "g1024"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_both_forms_read_back_to_the_frame(ctx, n, cut):
    meta = both_forms(ctx, edge_frame(n), **cut)
    assert meta.num_rows == n and meta.num_row_groups == (-(-n // 1024) if cut else min(n, 1))
    if n:
        emb, tok = meta.row_group(0).column(0), meta.row_group(0).column(1)
        assert emb.path_in_schema == "emb.list.element" and emb.num_values == 3 * min(n, 1024 if cut else n) and not emb.is_stats_set
        assert emb.encodings == ("PLAIN", "RLE") and tok.physical_type == "INT64" and meta.schema.column(0).max_definition_level == 3


def test_a_row_across_blocks_and_a_word_edge(ctx):
    """Rows of 9 000 elements: the second page starts at entry 10 023, bit 39 of a level word, and its long row runs over
    three 4 096-entry blocks; with null elements (the ranked path) and without (the straight copy)."""
    lens = np.ones(1030, dtype=np.int64)
    lens[[5, 1026]] = 9000
    frame = {"holes": lists("float64", lens, None, lambda e: e % 97 == 3), "dense": lists("float32", lens), "i": lists("int64", lens, lambda r: r == 1027, wide=True)}
    meta = both_forms(ctx, frame, rows_per_group=1024, page_bytes=4096)
    assert [meta.row_group(g).column(0).num_values for g in (0, 1)] == [10023, 9005]


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_a_frame_that_read_parquet_returned_is_written_back(ctx, form, wide):
    """write_parquet(read_parquet(x)): public `ListColumn`s with both bitmaps, as the reader leaves them, beside its flat `Column`s."""
    frame = edge_frame(1025)
    first = tabular.write_parquet(frame, ctx=ctx, rows_per_group=1024, page_bytes=4096)
    schema = {n: _capi.OXH_PARQUET_LIST | tabular._LIST_ELEMENT[str(c.values.dtype)] | (_capi.OXH_PARQUET_LIST64 if wide else 0)
              for n, c in frame.items() if isinstance(c, _ListCells)}
    if form == "host":
        back = tabular.read_parquet(first, schema=schema, ctx=ctx)
        again, stats = tabular.write_parquet(back, ctx=ctx, with_stats=True)
    else:
        back = tabular.read_parquet_device(torch.from_numpy(np.frombuffer(first, dtype=np.uint8).copy()).to("cuda:0"), schema=schema, ctx=ctx, stream=ctx.stream)
        again, stats = tabular.write_parquet_device(back, ctx=ctx, stream=ctx.stream, with_stats=True)
        again = again.cpu().numpy().tobytes()
    for n in schema:
        assert isinstance(back[n], tabular.ListColumn) and back[n].validity is not None and back[n].child_validity is not None
        assert str(back[n].offsets.dtype).endswith("int64" if wide else "int32")
    check(again, frame, stats)


def test_with_dictionaries_a_list_chunk_stays_plain(ctx):
    meta = both_forms(ctx, edge_frame(1025), dictionary=True, page_bytes=4096)
    assert meta.row_group(0).column(1).encodings == ("PLAIN", "RLE") and "RLE_DICTIONARY" in meta.row_group(0).column(5).encodings


@pytest.mark.parametrize("offsets, nvalues, what", [([0, 2, 1], 2, "a list column's offsets decrease or are negative"), ([0, 1, 2], 0, "has elements but no values"),
                                                   ([0, 1, 1 + (1 << 31)], 2, "more than INT32_MAX elements")], ids=["pair", "no-values", "long"])
def test_the_device_form_finds_bad_lists_after_the_measure(ctx, offsets, nvalues, what):
    """Nothing is read through such a list: the values tensor is far shorter than the long list's offsets say."""
    col = tabular.ListColumn(torch.zeros(nvalues, dtype=torch.int64, device="cuda:0"), torch.tensor(offsets, dtype=torch.int64, device="cuda:0"), None, None)
    with pytest.raises(_capi.OxenError, match=what):
        tabular.write_parquet_device({"v": col}, ctx=ctx, stream=ctx.stream)


def test_without_a_list_column_the_file_is_the_old_entry_s(ctx):
    frame, types = T.edge_frame(1025)
    head = tabular._parquet_head(frame, 1024, 4096, types)
    tables, child = tabular._parquet_tables(head[0], lambda a: None if a is None else a.ctypes.data)
    files = []
    for name, more in (("oxh_write_parquet_host", ()), ("oxh_write_parquet_lists_host", child)):
        fixed = (getattr(_capi.lib(), name), name, ctx, *head[:2], tables, *head[2:])
        need, _ = tabular._write_call(*fixed, None, 0, *more)
        out = np.zeros(need, dtype=np.uint8)
        assert tabular._write_call(*fixed, out.ctypes.data, need, *more)[0] == need
        files.append(out.tobytes())
    assert files[0] == files[1]


def test_snappy(ctx):
    meta = both_forms(ctx, edge_frame(1025), compression="snappy", page_bytes=4096)
    assert meta.row_group(0).column(1).compression == "SNAPPY"


def test_past_the_launch_caps(ctx):
    """300 000 rows of 60 elements, 18 M entries: more rows than the count kernel's 262 144 lanes, more words than the
    levels kernel's 4 096 runs of 32, more blocks than the emit kernel's 4 096 waves, more tiles than the tile kernel's
    256 waves. A null element in a thousand keeps every page on the ranked path."""
    frame = {"v": lists("float32", np.full(300000, 60), None, lambda e: e % 1000 == 7)}
    assert both_forms(ctx, frame).num_rows == 300000


@pytest.mark.parametrize("form", ["host", "device"])
def test_outputs_do_not_depend_on_what_the_scratch_held(ctx, form):
    """tests/test_parquet_write_scratch.py's twin: three poisons of the working memory, one file."""
    frame, how = edge_frame(3 * 1024 + 67), dict(ctx=ctx, with_stats=True, rows_per_group=2048, page_bytes=12000)
    device = {n: to_device(c) for n, c in frame.items()}
    seen = set()
    for poison in (0x00, 0xFF, 0x5A):
        assert _capi.lib().oxh_set_scratch_poison(poison) == -1
        try:
            before = _capi.lib().oxh_scratch_poisoned_bytes()
            data, stats = tabular.write_parquet(frame, **how) if form == "host" else tabular.write_parquet_device(device, stream=ctx.stream, **how)
            assert _capi.lib().oxh_scratch_poisoned_bytes() > before, "no working allocation was poisoned"
        finally:
            _capi.lib().oxh_set_scratch_poison(-1)
        seen.add((data if form == "host" else data.cpu().numpy().tobytes(), stats))
    assert len(seen) == 1, "the file depends on what the scratch or the output held"
    check(*seen.pop()[:1], frame, stats)
