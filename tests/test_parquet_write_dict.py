"""OXH_PARQUET_DICTIONARY on the GPU (`write_parquet(..., dictionary=True)`, oxen_amd/csrc/parquet_dict.hip): the file
decoded by plain Python -- tests/_parquet.py's Thrift values, levels and PLAIN bodies, and the bit-packed run here --
gives the frame bit for bit; the entries are distinct and in first-occurrence order, pad indices are 0, offsets, sizes
and encodings are what the pages say, a chunk past a limit is the PLAIN writer's chunk byte for byte."""
import struct

import numpy as np
import pytest

import _csvwrite_call as C
import _parquet as P
import _snappy_cases as S
import test_parquet_write as T
import test_parquet_write_snappy as TS
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
W = C.W
MAX_ENTRIES, MAX_CELL = 65536, 256   # kDictMaxEntries, kDictMaxCell
ONE_TILE = dict(rows_per_group=1024, page_bytes=4096)


def chunks_of(data):   # (meta, [(ColumnMetaData, [(page at, PageHeader, stored body)])]); the file ends at the footer
    meta_at = len(data) - 8 - struct.unpack_from("<I", data, len(data) - 8)[0]
    meta, end = P.value(data, meta_at, 12)
    assert data[:4] == b"PAR1" == data[-4:] and end == len(data) - 8
    at, out = 4, []
    for g in meta.get(4, []):
        assert g[5] == at
        for chunk in g[1]:
            md, pages, seen, start = chunk[3], [], 0, at
            while seen < md[5]:
                head, body_at = P.value(data, at, 12)
                pages.append((at, head, data[body_at:body_at + head[3]]))
                at, seen = body_at + head[3], seen + (head[5][1] if head[1] == 0 else 0)
            assert len(pages[-1][2]) == pages[-1][1][3] and md[7] == at - start and md[5] == g[3]
            out.append((md, pages))
        assert g[6] == sum(c[3][7] for c in g[1])
    assert at == meta_at
    return meta, out


def decode(data, ptypes):   # per column (validity, cells) and whether each chunk has a dictionary, of an uncompressed file
    parts, coded = [[] for _ in ptypes], []
    for k, (md, pages) in enumerate(chunks_of(data)[1]):
        t, entries, seen = ptypes[k % len(ptypes)], None, []
        if pages[0][1][1] == 2:   # DICTIONARY_PAGE: the chunk's first page, PLAIN entries
            at, head, body = pages.pop(0)
            entries = P.plain(t, body, head[7][1])
            keys = entries if isinstance(entries, list) else entries.tolist()
            assert md[11] == at and head[2] == head[3] <= 1 << 20 and head[7][2] == 0 and 1 <= len(keys) == len(set(keys)) <= MAX_ENTRIES
            w = max(1, (len(keys) - 1).bit_length())
        assert md[9] == pages[0][0] and md[6] == md[7] and (11 in md) == (entries is not None)
        assert md[2] == ([0, 3] if entries is None else [0, 3, 8])
        for at, head, body in pages:
            run = struct.unpack_from("<I", body, 0)[0]
            valid = P.levels(body[4:4 + run], head[5][1])
            nv, vals = int(valid.sum()), body[4 + run:]
            assert head[1] == 0 and head[2] == head[3] and head[5][2] == (0 if entries is None else 8)
            if entries is None:
                parts[k % len(ptypes)].append((valid, P.plain(t, vals, nv)))
                continue
            idx = np.zeros(0, dtype=np.int64)
            assert vals[0] == w and (nv or len(vals) == 1)
            if nv:   # one bit-packed run: ceil(nv / 8) groups of 8 indices, LSB first
                run_head, p = P.varint(vals, 1)
                assert run_head == ((nv + 7) // 8 << 1) | 1 and len(vals) == p + (nv + 7) // 8 * w
                bits = np.unpackbits(np.frombuffer(vals[p:], dtype=np.uint8), bitorder="little").reshape(-1, w).astype(np.int64)
                idx = (bits << np.arange(w)).sum(axis=1)
                assert not idx[nv:].any(), "a pad index is not 0"
            seen.append(idx[:nv])
            parts[k % len(ptypes)].append((valid, [entries[i] for i in idx[:nv]] if isinstance(entries, list) else entries[idx[:nv]]))
        if entries is not None:   # every entry is used, and entry k's first use comes before entry k + 1's
            _, firsts = np.unique(np.concatenate(seen), return_index=True)
            assert len(firsts) == len(keys) and np.all(np.diff(firsts) > 0)
        coded.append(entries is not None)
    cat = lambda arrays, dtype: np.concatenate(arrays) if arrays else np.zeros(0, dtype=dtype)  # noqa: E731
    return [(cat([v for v, _ in col], bool), [x for _, cells in col for x in cells] if t == P.BYTE_ARRAY else
             cat([x for _, x in col], bool if t == P.BOOLEAN else "<u8")) for t, col in zip(ptypes, parts)], coded


def sizes(n):   # a column name starting with "p" stays PLAIN; the nulls leave every row group's first row valid
    nan = [struct.unpack("<d", struct.pack("<Q", b))[0] for b in (0x7FF8000000000001, 0xFFF8000000000002)]
    prefix = b"0123456789abcdef"
    spec = [("d1", W.INT64, [7] * n), ("d2", W.INT64, [r % 2 for r in range(n)]), ("d3", W.INT64, [-(r % 3) for r in range(n)]),
            ("d256", W.INT64, [None if r % 7 == 3 else r % 256 for r in range(n)]), ("d257", W.FLOAT64, [float(r % 257) for r in range(n)]),
            ("p_allnull", W.INT64, [None] * n), ("tile_end", W.INT64, [r if r % 1024 == 1023 else 0 for r in range(n)]),
            ("high", W.INT64, [1 + ((r % 3) << 40) for r in range(n)]), ("zeros_nans", W.FLOAT64, [[-0.0, 0.0, nan[0], nan[1]][r % 4] for r in range(n)]),
            ("third_null", W.STRING, [None if r % 1024 % 3 == 1 else b"label-%d" % (r % 5) for r in range(n)]),
            ("empty", W.STRING64, [[b"", None, b"a"][r % 1024 % 3] for r in range(n)]), ("shared", W.STRING, [prefix + bytes([65 + r % 4]) for r in range(n)]),
            ("p_bool", W.BOOL, [None if r % 5 == 4 else r % 3 == 0 for r in range(n)])]
    return {name: C.host_column(t, cells, nbit=1) for name, t, cells in spec}, [t for _, t, _ in spec]


def entries():   # kDictMaxEntries distinct values, and one more
    n = MAX_ENTRIES + 1
    spec = [("most", W.INT64, [r % MAX_ENTRIES for r in range(n)]), ("p_more", W.INT64, list(range(n))), ("p_bool", W.BOOL, [r % 2 == 0 for r in range(n)])]
    return {name: C.host_column(t, cells) for name, t, cells in spec}, [t for _, t, _ in spec]


def cells():   # a cell at and past kDictMaxCell; 4 096 and 4 097 entries of 4 + 252 bytes: a dictionary page of 1 MiB and just over
    n, wide = 4200, lambda r: b"%0252d" % r   # noqa: E731
    spec = [("longest", W.STRING, [b"x" * MAX_CELL if r % 2 else b"y" for r in range(n)]), ("p_longer", W.STRING, [b"x" * (MAX_CELL + (r == 4100)) for r in range(n)]),
            ("mib", W.STRING, [wide(r % 4096) for r in range(n)]), ("p_over_mib", W.STRING64, [wide(r % 4097) for r in range(n)])]
    return {name: C.host_column(t, cells) for name, t, cells in spec}, [t for _, t, _ in spec]


FRAMES = {**{"n%d%s" % (n, "_one_tile" if cut else ""): ((lambda n=n: sizes(n)), cut) for n in (0, 1, 1023, 1025, 2049) for cut in ({}, ONE_TILE)},
          "entries": (entries, {}), "cells": (cells, {})}


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_the_file_decodes_to_the_frame(ctx, name, form):
    (frame, types), cut = FRAMES[name][0](), FRAMES[name][1]
    data, stats = TS.write(ctx, frame, types, form, dictionary=True, **cut)
    plain, _ = TS.write(ctx, frame, types, form, dictionary=False, **cut)
    assert plain == TS.write(ctx, frame, types, form, **cut)[0]   # the flag clear: the file of a call without the argument
    got, coded = decode(data, [T.PARQUET_TYPE[t] for t in types])
    want = [T.cells_of(c) for c in frame.values()]
    ngroups = len(coded) // len(types)
    assert coded == [not n.startswith("p") for n in frame] * ngroups
    assert tuple(stats) == (len(data), ngroups, sum(len(pages) for _, pages in chunks_of(data)[1]), sum(int((~v).sum()) for v, _ in want))
    with tabular.ParquetFile(data, ctx=ctx) as f:
        back, column_stats = f.columns(range(len(types)), [t.type for t in f.types()], with_stats=True)
    assert sum(s.dict_values for s in column_stats) > 0 or not any(coded)
    for columns in [got, [T.cells_of(c) for c in back]] + T.pyarrow_columns(data):
        for (valid, values), (wvalid, wvalues), column in zip(columns, want, frame):
            assert np.array_equal(valid, wvalid) and (values == wvalues if isinstance(wvalues, list) else np.array_equal(values, wvalues)), column
    raw = lambda d: [d[pages[0][0]:pages[0][0] + md[7]] for md, pages in chunks_of(d)[1]]   # noqa: E731
    for k, (mine, theirs) in enumerate(zip(raw(data), raw(plain))):   # a chunk without a dictionary is the PLAIN writer's chunk
        assert coded[k] or mine == theirs, list(frame)[k % len(types)]


def test_identical_bytes_from_both_forms_and_two_runs(ctx):
    frame, types = sizes(2049)
    files = [TS.write(ctx, frame, types, form, dictionary=True, compression=codec, **ONE_TILE) for codec in (None, "snappy") for form in ("host", "device", "device")]
    assert files[0] == files[1] == files[2] and files[3] == files[4] == files[5]


@pytest.mark.parametrize("name", ["n2049_one_tile", "cells"])
def test_snappy_bodies_inflate_to_the_dictionary_file(ctx, name):
    (frame, types), cut = FRAMES[name][0](), FRAMES[name][1]
    twin, _ = TS.write(ctx, frame, types, "device", dictionary=True, **cut)
    data, stats = TS.write(ctx, frame, types, "device", dictionary=True, compression="snappy", **cut)
    (meta, packed), (tmeta, plain) = chunks_of(data), chunks_of(twin)
    assert stats.bytes == len(data) and meta[2] == tmeta[2] and len(packed) == len(plain)
    for (md, pages), (tmd, tpages) in zip(packed, plain):
        assert md[4] == 1 and md[2] == tmd[2] and (md.get(11) is None) == (tmd.get(11) is None) and len(pages) == len(tpages)
        assert md[9] == pages[1 if 11 in md else 0][0] and md.get(11, pages[0][0]) == pages[0][0] and md[6] - md[7] == sum(h[2] - h[3] for _, h, _ in pages)
        for (_, head, body), (_, thead, tbody) in zip(pages, tpages):
            assert head[1] == thead[1] and head[2] == thead[2] == len(tbody) and head.get(7) == thead.get(7) and S.inflate(body, head[2]) == tbody
    with pytest.raises(_capi.OxenError, match="out holds %d B, the file has" % len(data)):   # the first call's size is a bound above the file's
        tabular.write_parquet_device({n: C.to_device(c) for n, c in frame.items()}, types=types, ctx=ctx, stream=ctx.stream, capacity=len(data), dictionary=True,
                                     compression="snappy", **cut)


def test_smaller_than_plain_and_unknown_flags(ctx, monkeypatch):
    frame, types = TS.wide()
    frame, types = {n: frame[n] for n in ("steps", "text")}, types[1:]   # 400 and 1 000 values against 8 and 14 bytes a cell
    assert len(tabular.write_parquet(frame, types=types, ctx=ctx, dictionary=True)) < len(tabular.write_parquet(frame, types=types, ctx=ctx))
    monkeypatch.setattr(_capi, "OXH_PARQUET_DICTIONARY", 8)
    with pytest.raises(_capi.OxenError, match="unknown flags"):
        tabular.write_parquet(frame, types=types, ctx=ctx, dictionary=True)
