"""OXH_PARQUET_SNAPPY on the GPU (oxh_write_parquet_* with the flag, `compression="snappy"`): the compressed file walked
page by page beside its uncompressed twin -- every body inflates, by the plain decoder of tests/_snappy_cases.py, to the
twin's body; headers, chunk and row-group sizes are the sums of what is stored; the file ends at the footer --, the
readers, and the sizing contract (a bound first, the size after)."""
import ctypes
import io
import struct

import numpy as np
import pytest

import _csvwrite_call as C
import _parquet as P
import _snappy_cases as S
import test_parquet_write as T
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
W = C.W


def wide(n=40000):   # pages of several fragments: 320 000 B of random int64, a compressible twin, strings
    rng = np.random.default_rng(4)
    spec = [("noise", W.INT64, [int(v) for v in rng.integers(-1 << 62, 1 << 62, n)]), ("steps", W.INT64, [r // 100 for r in range(n)]),
            ("text", W.STRING, [None if r % 50 == 7 else b"row-%06d" % (r % 1000) for r in range(n)])]
    return {name: C.host_column(t, cells) for name, t, cells in spec}, [t for _, t, _ in spec]


def huge():   # one cell above 128 KiB: a page of 3 fragments and more
    cells = [b"small", b"the quick brown fox " * 10000, None, b"\x00" * 70000] + [b"tail-%d" % r for r in range(1100)]
    return {"s": C.host_column(W.STRING, cells), "b": C.host_column(W.BOOL, [r % 7 == 0 for r in range(len(cells))])}, [W.STRING, W.BOOL]


FRAMES = {"edges": (lambda: T.edge_frame(2049), {}), "edges_one_tile_pages": (lambda: T.edge_frame(2049), dict(rows_per_group=1024, page_bytes=4096)),
          "no_rows": (lambda: T.edge_frame(0), {}), "fragments": (wide, {}), "fragments_in_groups": (wide, dict(rows_per_group=16384, page_bytes=1 << 18)),
          "huge_cell": (huge, {})}


def write(ctx, frame, types, form, **kw):
    if form == "host":
        return tabular.write_parquet(frame, types=types, ctx=ctx, with_stats=True, **kw)
    data, stats = tabular.write_parquet_device({n: C.to_device(c) for n, c in frame.items()}, types=types, ctx=ctx, stream=ctx.stream, with_stats=True, **kw)
    return data.cpu().numpy().tobytes(), stats


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_compressed_file_beside_its_twin(ctx, name, form):
    (frame, types), cut = FRAMES[name][0](), FRAMES[name][1]
    twin, _ = write(ctx, frame, types, form, **cut)
    data, stats = write(ctx, frame, types, form, compression="snappy", **cut)
    f = P.read(twin)
    assert data[:4] == b"PAR1" == data[-4:] and stats.bytes == len(data) and tuple(stats)[1:] == (len(f.groups), sum(len(c["pages"]) for g in f.groups for c in g["chunks"]), stats.nulls)
    meta_at = len(data) - 8 - struct.unpack_from("<I", data, len(data) - 8)[0]
    meta, end = P.value(data, meta_at, 12)
    assert end == len(data) - 8 and meta[2] == f.meta[2] and meta[3] == f.num_rows and len(meta.get(4, [])) == len(f.groups)
    at = 4
    for g, tg, traw in zip(meta.get(4, []), f.groups, f.meta.get(4, [])):
        assert g[5] == at and g[3] == tg["rows"]
        for chunk, tc, tchunk in zip(g[1], tg["chunks"], traw[1]):
            md, stored, plain = chunk[3], 0, 0
            assert md[4] == 1 and md[9] == at and md[5] == tchunk[3][5] and md.get(12) == tchunk[3].get(12) and md[2] == tchunk[3][2]
            for t_at, t_head_len, t_body_len, rows in tc["pages"]:
                head, body_at = P.value(data, at, 12)
                t_head, _ = P.value(twin, t_at, 12)
                assert head[1] == t_head[1] == 0 and head[5] == t_head[5] and head[2] == t_body_len and head[3] > 0
                body = data[body_at:body_at + head[3]]
                assert len(body) == head[3] and S.inflate(body, head[2]) == twin[t_at + t_head_len:t_at + t_head_len + t_body_len]
                stored, plain, at = stored + body_at - at + head[3], plain + body_at - at + head[2], body_at + head[3]
            assert (md[7], md[6]) == (stored, plain)
        assert g[6] == sum(c[3][7] for c in g[1]) and g[2] == sum(c[3][6] for c in g[1])
    assert at == meta_at   # the file ends exactly at the footer
    if name != "no_rows":
        assert len(data) < len(twin)   # every frame here has something to compress
    want = [T.cells_of(c) for c in frame.values()]
    got = [[T.cells_of(c) for c in tabular.read_parquet(data, ctx=ctx).values()]] + T.pyarrow_columns(data)
    for columns in got:
        for (valid, values), (wvalid, wvalues), column in zip(columns, want, frame):
            assert np.array_equal(valid, wvalid) and (values == wvalues if isinstance(wvalues, list) else np.array_equal(values, wvalues)), column
    try:
        import pyarrow.parquet as pq
    except ImportError:
        return
    groups = pq.ParquetFile(io.BytesIO(data)).metadata
    assert all(groups.row_group(0).column(c).compression == "SNAPPY" for c in range(len(frame)) if groups.num_row_groups)


def test_identical_bytes_from_both_forms(ctx):
    frame, types = wide()
    assert write(ctx, frame, types, "host", compression="snappy") == write(ctx, frame, types, "device", compression="snappy")


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_bound_first_the_size_after(ctx, form):
    """An incompressible string column through the C entry with a buffer of guard bytes: the measure-only call gives a
    capacity, not the size; one byte less is the error with out untouched and the bound in out_bytes and stats4[0]; the
    capacity itself suffices, the file grows beside its twin and nothing behind it is written."""
    import torch

    rng = np.random.default_rng(8)
    col = C.host_column(W.STRING, [rng.integers(0, 256, 700, dtype=np.uint8).tobytes() for _ in range(1500)])
    twin = tabular.write_parquet({"s": col}, types=[W.STRING], ctx=ctx)
    cols = [C.to_device(col)] if form == "device" else [col]
    keep = []

    def ptr(a):
        if a is None:
            return None
        if form == "device":
            return a.data_ptr() if a.numel() else None
        keep.append(np.ascontiguousarray(a))
        return keep[-1].ctypes.data if keep[-1].size else None

    tables = tabular._tables(cols, ptr)
    names, name_offsets = np.frombuffer(b"s\0", dtype=np.uint8), np.array([0, 1], dtype=np.uint64)
    size, stats = ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
    fn = _capi.lib().oxh_write_parquet_device if form == "device" else _capi.lib().oxh_write_parquet_host

    def call(out, capacity):
        tail = (ctx.stream,) if form == "device" else ()
        rc = fn(ctx.handle, 1500, 1, (ctypes.c_uint32 * 1)(W.STRING), *tables, names.ctypes.data, name_offsets.ctypes.data_as(_capi._u64p), 0, 0,
                _capi.OXH_PARQUET_SNAPPY, out, capacity, ctypes.byref(size), stats, *tail)
        return rc, int(size.value), int(stats[0])

    rc, bound, first = call(None, 0)
    assert rc == _capi.OXH_OK and bound == first > len(twin)
    guard = np.full(bound + 64, S.GUARD, dtype=np.uint8)
    buf = torch.from_numpy(guard.copy()).to("cuda:0") if form == "device" else guard.copy()
    at = buf.data_ptr() if form == "device" else buf.ctypes.data
    back = lambda: buf.cpu().numpy() if form == "device" else buf  # noqa: E731
    assert call(at, bound - 1) == (_capi.OXH_ERR_INVALID, bound, bound) and b"out holds %d B, the file has %d" % (bound - 1, bound) in _capi.lib().oxh_last_error()
    assert np.array_equal(back(), guard), "a refused call wrote to out"
    rc, actual, reported = call(at, bound)
    assert rc == _capi.OXH_OK and actual == reported and len(twin) < actual <= bound   # a V1 page of a SNAPPY chunk is compressed also when it grows
    data = back()
    assert np.all(data[actual:] == S.GUARD) and data[:actual].tobytes() == tabular.write_parquet({"s": col}, types=[W.STRING], ctx=ctx, compression="snappy")
