"""A plain reader for the Parquet subset oxh_write_parquet_* writes (include/oxen_hash.h "Parquet"), without the
library: a Thrift-compact decoder into {field id: value}, the footer, the page walk, levels and PLAIN values back to
(validity, values) per column, the row-group and page boundaries and the statistics. Sizes and offsets are checked
against the bytes (AssertionError). tests/test_parquet_write_cpu.py pins it on files pyarrow wrote."""
import struct
import types

import numpy as np

BOOLEAN, INT64, DOUBLE, BYTE_ARRAY = 0, 2, 5, 6


def varint(b, p):
    v = shift = 0
    while True:
        v |= (b[p] & 0x7F) << shift
        shift += 7
        p += 1
        if not b[p - 1] & 0x80:
            return v, p


def value(b, p, t):   # one value of compact type t: a boolean (in the field header), an integer, binary, list, struct
    if t in (1, 2):
        return t == 1, p
    if t in (4, 5, 6):
        v, p = varint(b, p)
        return (v >> 1) ^ -(v & 1), p
    if t == 8:
        n, p = varint(b, p)
        return bytes(b[p:p + n]), p + n
    if t == 9:
        n, et = b[p] >> 4, b[p] & 15
        p += 1
        if n == 15:
            n, p = varint(b, p)
        items = []
        for _ in range(n):
            v, p = value(b, p, et)
            items.append(v)
        return items, p
    assert t == 12, f"thrift type {t}"
    out, last = {}, 0
    while b[p]:
        head = b[p]
        last, p = (last + (head >> 4), p + 1) if head >> 4 else value(b, p + 1, 4)
        out[last], p = value(b, p, head & 15)
    return out, p + 1


def levels(b, n):   # the n definition levels of one hybrid stream at width 1, as booleans; pad bits must be 0
    out, p = np.zeros(0, dtype=bool), 0
    while out.size < n:
        head, p = varint(b, p)
        if head & 1:
            bits = np.unpackbits(np.frombuffer(b[p:p + (head >> 1)], dtype=np.uint8), bitorder="little").astype(bool)
            assert bits.size == 8 * (head >> 1)
            p += head >> 1
        else:
            assert b[p] in (0, 1)
            bits = np.full(head >> 1, bool(b[p]))
            p += 1
        out = np.concatenate([out, bits])
    assert p == len(b) and not out[n:].any(), "bytes behind the levels' last run, or pad bits set"
    return out[:n]


def plain(ptype, b, nvalid):
    if ptype in (INT64, DOUBLE):
        assert len(b) == 8 * nvalid, (len(b), nvalid)
        return np.frombuffer(b, dtype="<u8")          # the bits: a NaN or -0.0 compares as written
    if ptype == BOOLEAN:
        bits = np.unpackbits(np.frombuffer(b, dtype=np.uint8), bitorder="little").astype(bool)
        assert len(b) == (nvalid + 7) // 8 and not bits[nvalid:].any(), "the booleans' size, or pad bits set"
        return bits[:nvalid]
    cells, p = [], 0
    for _ in range(nvalid):
        n = struct.unpack_from("<I", b, p)[0]
        cells.append(bytes(b[p + 4:p + 4 + n]))
        p += 4 + n
    assert ptype == BYTE_ARRAY and p == len(b), "bytes behind the last cell"
    return cells


def read(data: bytes):
    """A namespace of names, types (Parquet's), schema and meta (raw), num_rows, created_by, columns [(validity,
    values)] and groups [{rows, chunks: [{pages: [(offset, header bytes, body bytes, rows)], null_count, min, max}]}]."""
    f = types.SimpleNamespace()
    assert data[:4] == b"PAR1" == data[-4:] and len(data) >= 12
    meta_at = len(data) - 8 - struct.unpack_from("<I", data, len(data) - 8)[0]
    f.meta, end = value(data, meta_at, 12)
    assert end == len(data) - 8, "the footer's length is not its bytes"
    f.schema, f.names, f.types = f.meta[2], [s[4] for s in f.meta[2][1:]], [s[1] for s in f.meta[2][1:]]
    assert f.schema[0][5] == len(f.schema) - 1 and f.schema[0].get(1) is None
    f.num_rows, f.created_by = f.meta[3], f.meta.get(6)
    parts, f.groups, at = [[] for _ in f.types], [], 4
    for g in f.meta.get(4, []):
        group = {"rows": g[3], "chunks": []}
        assert len(g[1]) == len(f.types) and g[5] == at, "a row group starts where the one before ended"
        for c, chunk in enumerate(g[1]):
            md = chunk[3]
            assert md[1] == f.types[c] and sorted(md[2]) == [0, 3] and md[3] == [f.names[c]] and md[4] == 0 and md[5] == g[3] and md[9] == at and md[6] == md[7], (at, md)
            pages, nulls, seen = [], 0, 0
            while seen < md[5]:
                head, body_at = value(data, at, 12)
                n, body = head[5][1], data[body_at:body_at + head[2]]
                assert head[1] == 0 and head[2] == head[3] == len(body) and head[5][2] == 0 and head[5][3] == 3, head
                run = struct.unpack_from("<I", body, 0)[0]
                valid = levels(body[4:4 + run], n)
                parts[c].append((valid, plain(f.types[c], body[4 + run:], int(valid.sum()))))
                pages.append((at, body_at - at, head[2], n))
                at, seen, nulls = body_at + head[2], seen + n, nulls + n - int(valid.sum())
            stats = md.get(12, {})
            assert seen == md[5] and at - md[9] == md[6] and stats.get(3) == nulls, (md, at, nulls)
            group["chunks"].append({"pages": pages, "null_count": nulls, "min": stats.get(6), "max": stats.get(5)})
        assert g[2] == g[6] == sum(ch[3][6] for ch in g[1])
        f.groups.append(group)
    assert sum(g["rows"] for g in f.groups) == f.num_rows and at == meta_at, "rows, or bytes between the last page and the footer"
    cat = lambda arrays, dtype: np.concatenate(arrays) if arrays else np.zeros(0, dtype=dtype)  # noqa: E731
    f.columns = [(cat([v for v, _ in col], bool), [x for _, cells in col for x in cells] if t == BYTE_ARRAY else
                  cat([x for _, x in col], bool if t == BOOLEAN else "<u8")) for t, col in zip(f.types, parts)]
    return f
