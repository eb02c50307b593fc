"""The Parquet writer on the GPU (oxh_write_parquet_*, oxen_amd/csrc/parquet_write.hip): `write_parquet` and
`write_parquet_device` give identical bytes that read back -- by tests/_parquet.py, which also checks the metadata's
offsets and sizes, and by pyarrow where it imports -- to the frame cell for cell, with numpy's statistics. The shapes
are the smallest that reach every path: wave, tile, pages and groups of one and two tiles, bit offsets, the LDS span
and the long-cell threshold of the strings, the launch cap."""
import io
import os

import numpy as np
import pytest

import _csvwrite_call as C
import _parquet as P
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu
W = C.W
PARQUET_TYPE = {W.INT64: P.INT64, W.FLOAT64: P.DOUBLE, W.BOOL: P.BOOLEAN, W.STRING: P.BYTE_ARRAY, W.STRING64: P.BYTE_ARRAY}


def cells_of(col):
    """(validity as booleans, the valid cells: the bits of 8-byte values, booleans, or a list of bytes) of a host Column."""
    n = col.nrows
    bits = lambda a, at: np.unpackbits(np.asarray(a, dtype=np.uint8), bitorder="little")[at:at + n].astype(bool)  # noqa: E731
    valid = np.ones(n, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit)
    if col.kind == _capi.OXH_COL_BOOL:
        return valid, bits(col.values, col.value_bit)[valid]
    if col.kind == _capi.OXH_COL_FIXED8:
        return valid, np.ascontiguousarray(col.values).view("<u8")[valid]
    raw, offsets = np.asarray(col.values).tobytes(), np.asarray(col.offsets)
    return valid, [raw[int(offsets[r]):int(offsets[r + 1])] for r in np.flatnonzero(valid)]


def pyarrow_columns(data):   # [the file as pyarrow.parquet.read_table gives it, in cells_of's form], [] without pyarrow
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq
    except ImportError:
        return []
    out = []
    for arr in pq.read_table(io.BytesIO(data)).columns:
        valid, arr = ~np.asarray(arr.combine_chunks().is_null()), arr.combine_chunks().drop_null()
        v = arr.cast(pa.binary()).to_pylist() if pa.types.is_string(arr.type) else arr.to_numpy(zero_copy_only=False)
        out.append((valid, v if isinstance(v, list) or v.dtype == bool else v.view("<u8")))
    return [out]


def check(data, stats, cols, types, names):
    """The file against the frame by both readers, every chunk's statistics against numpy's, stats4; returns the file."""
    f = P.read(data)
    assert f.names == list(names) and f.types == [PARQUET_TYPE[t] for t in types] and f.num_rows == cols[0].nrows and b"oxen_amd" in f.created_by
    for s, t in zip(f.schema[1:], types):
        assert s[3] == 1 and (s.get(6), s.get(10)) == ((0, {1: {}}) if PARQUET_TYPE[t] == P.BYTE_ARRAY else (None, None))
    want = [cells_of(c) for c in cols]
    for got in [f.columns] + pyarrow_columns(data):
        for (valid, values), (wvalid, wvalues), name in zip(got, want, names):
            assert np.array_equal(valid, wvalid) and (values == wvalues if isinstance(wvalues, list) else np.array_equal(values, wvalues)), name
    row0 = 0
    for k, g in enumerate(f.groups):
        for c, (chunk, (valid, values), t) in enumerate(zip(g["chunks"], want, types)):
            assert f.meta[4][k][1][c][3][2] == [0, 3] and chunk["null_count"] == int((~valid[row0:row0 + g["rows"]]).sum())
            lo = hi = None
            if t in (W.INT64, W.FLOAT64):
                v = values[int(valid[:row0].sum()):int(valid[:row0 + g["rows"]].sum())]
                v = v.view("<i8") if t == W.INT64 else v.view("<f8")[~np.isnan(v.view("<f8"))]
                if v.size and t == W.INT64:
                    lo, hi = v.min().tobytes(), v.max().tobytes()
                elif v.size:   # the format's rule: a zero min is -0.0, a zero max +0.0
                    lo, hi = (v.min() if v.min() else np.float64(-0.0)).tobytes(), (v.max() if v.max() else np.float64(0.0)).tobytes()
            assert (chunk["min"], chunk["max"]) == (lo, hi), (t, chunk, lo, hi)
        row0 += g["rows"]
    npages = sum(len(c["pages"]) for g in f.groups for c in g["chunks"])
    assert stats == (len(data), len(f.groups), npages, sum(int((~v).sum()) for v, _ in want)), stats
    return f


def both_forms(ctx, frame, types, **cut):   # frame: {name: host Column}; identical bytes from both forms, checked once
    names, cols = list(frame), list(frame.values())
    host, stats = tabular.write_parquet(frame, types=types, ctx=ctx, with_stats=True, **cut)
    dev, dstats = tabular.write_parquet_device({n: C.to_device(c) for n, c in frame.items()}, types=types, ctx=ctx, stream=ctx.stream,
                                               with_stats=True, **cut)
    assert dev.cpu().numpy().tobytes() == host and tuple(dstats) == tuple(stats)
    return check(host, tuple(stats), cols, types, [n.encode() for n in names])


def edge_frame(n):   # every column type under every validity shape, at n rows
    alt = lambda cells: [None if r % 2 else c for r, c in enumerate(cells)]  # noqa: E731
    edges = {63, 64, 1023, 1024, 127, 128}                                     # a null on each side of a word and of a tile edge
    ints = [[-(1 << 63), (1 << 63) - 1, 0, -1, r][r % 5] for r in range(n)]
    floats = [[0.5, -0.0, float("nan"), 0.0, float("inf"), float("-inf"), -2.5e300][r % 7] for r in range(n)]
    bools = [r % 3 == 0 for r in range(n)]
    strings = [b"x" * [0, 1, 15, 16, 17][r % 5] + b"\xff" * (r % 2) for r in range(n)]   # invalid UTF-8 is copied as it is
    spec = [
        ("i_plain", W.INT64, ints, {}), ("i_alt", W.INT64, alt(ints), dict(nbit=1)), ("i_edges", W.INT64, [None if r in edges else v for r, v in enumerate(ints)], {}),
        ("i_allvalid", W.INT64, ints, dict(validity="always", nbit=7)), ("i_allnull", W.INT64, [None] * n, {}),
        ("f_mixed", W.FLOAT64, [None if r % 9 == 4 else v for r, v in enumerate(floats)], dict(nbit=7)), ("f_nan", W.FLOAT64, [float("nan")] * n, {}),
        ("f_zero", W.FLOAT64, [[-0.0, 0.0][r % 2] for r in range(n)], {}),
        ("b_plain", W.BOOL, bools, dict(vbit=1)), ("b_alt", W.BOOL, alt(bools), dict(vbit=7, nbit=1)),
        ("b_edges", W.BOOL, [None if r in edges or r % 10 == 9 else v for r, v in enumerate(bools)], dict(nbit=7)), ("b_allnull", W.BOOL, [None] * n, {}),
        ("s_plain", W.STRING, strings, dict(lead=b"lead")), ("s_alt", W.STRING64, alt(strings), dict(nbit=1)),
        ("s_edges", W.STRING, [None if r in edges else v for r, v in enumerate(strings)], {}),
    ]
    return {name: C.host_column(t, cells, **kw) for name, t, cells, kw in spec}, [t for _, t, _, _ in spec]


@pytest.mark.parametrize("cut", [{}, dict(rows_per_group=1024, page_bytes=4096), dict(rows_per_group=2048, page_bytes=4096)], ids=["default", "g1024", "g2048"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_both_forms_read_back_to_the_frame(ctx, n, cut):
    frame, types = edge_frame(n)
    f = both_forms(ctx, frame, types, **cut)
    group = cut.get("rows_per_group", 1 << 20)
    assert [g["rows"] for g in f.groups] == [min(group, n - at) for at in range(0, n, group)]
    if cut and n >= 1024:
        pages = {name: [p[3] for p in c["pages"]] for name, c in zip(frame, f.groups[0]["chunks"])}
        assert pages["i_plain"][0] == 1024 and pages["b_plain"] == [min(group, n)]   # a one-tile page; booleans fill the group's


@pytest.mark.parametrize("offsets", [W.STRING, W.STRING64], ids=["int32", "int64"])
def test_string_cells_around_the_lds_span_and_the_page(ctx, offsets):
    """Cells on both sides of the whole-wave threshold (4 + 508 = 512), one just past the LDS span (4 + 8 189), waves
    whose short cells overflow the span (64 x 204 bytes: runs), one cell larger than page_bytes, nulls between them."""
    n = 1024 + 130
    cells = [bytes([65 + r % 26]) * [3, 200, 0, 507, 508][r % 5] for r in range(n)]
    cells[70], cells[700], cells[1100] = b"s" * 8189, b"p" * 10000, b"q" * 8188
    for r in (0, 69, 71, 701, 1024):
        cells[r] = None
    frame = {"s": C.host_column(offsets, cells, nbit=1), "t": C.host_column(offsets, [b"y" * 200] * n, lead=b"0123456")}
    f = both_forms(ctx, frame, [offsets, offsets], rows_per_group=1024, page_bytes=4096)
    assert [len(c["pages"]) for c in f.groups[0]["chunks"]] == [1, 1] and f.groups[0]["chunks"][0]["pages"][0][2] > 100000


def test_past_the_launch_cap(ctx):
    """513 tiles x 8 columns: more items than the 4 096 waves of a capped launch; random nulls, default pages."""
    n, rng = 513 * 1024 + 5, np.random.default_rng(11)
    bits = lambda p: np.packbits(rng.random(n) < p, bitorder="little")  # noqa: E731
    offsets = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(rng.integers(0, 6, n), out=offsets[1:])
    cols = [Column(_capi.OXH_COL_FIXED8, n, rng.integers(-(1 << 63), (1 << 63) - 1, n), None, bits(0.9)),
            Column(_capi.OXH_COL_FIXED8, n, rng.standard_normal(n)), Column(_capi.OXH_COL_BOOL, n, bits(0.5), None, bits(0.01)),
            Column(_capi.OXH_COL_BYTES32, n, rng.integers(97, 123, int(offsets[-1])).astype(np.uint8), offsets, bits(0.9))] * 2
    f = both_forms(ctx, dict(zip("abcdefgh", cols)), [W.INT64, W.FLOAT64, W.BOOL, W.STRING] * 2)
    assert len(f.groups) == 1 and len(f.groups[0]["chunks"][0]["pages"]) > 3


def test_the_chain_over_a_fixture(ctx, tmp_path):
    """read_csv_device -> write_parquet_device on a golden CSV reads back; the host form writes the same to a path."""
    import torch

    data = open(os.path.join(os.path.dirname(__file__), "golden", "data_test", "csvs", "mixed_data_types.csv"), "rb").read()
    frame = tabular.read_csv_device(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0"), ctx=ctx, stream=ctx.stream)
    text, stats = tabular.write_parquet_device(frame, ctx=ctx, stream=ctx.stream, with_stats=True)
    host = {n: Column(c.kind, c.nrows, *(None if x is None else x.cpu().numpy() for x in (c.values, c.offsets, c.validity)), c.value_bit, c.validity_bit)
            for n, c in frame.items()}
    types = tabular._write_types(list(host), list(host.values()), None)
    check(text.cpu().numpy().tobytes(), tuple(stats), list(host.values()), types, [n.encode() for n in host])
    assert tabular.write_parquet(host, tmp_path / "x.parquet", ctx=ctx) == text.cpu().numpy().tobytes() == (tmp_path / "x.parquet").read_bytes()
