"""The CPU restatement the take tests compare with (tests/test_take.py, test_take_cpu.py): the take of
Arrow columns by two index arrays with a fallback source, in plain numpy, by the text of
include/oxen_hash.h. Columns are `oxen_amd.tabular.Column` descriptions over numpy arrays; nothing here
calls the library.

Cell (o, i) of output column o = (a, ia, b, ib): the cell of column a at idx[ia][i] if that index is present
and the cell valid; else the cell of column b at idx[ib][i] if b is there, that index present and the cell
valid; else null. The output buffers are fully defined, so they are compared byte for byte:
    validity     ceil(n / 8) bytes, LSB first, pad bits 0
    fixed width  n * width bytes, a null cell's bytes 0
    boolean      ceil(n / 8) bytes, null cells and pad bits 0
    bytes        n + 1 offsets of the column's own width from 0, the values tightly packed, a null cell empty
"""
from typing import Any, NamedTuple

import numpy as np

FIXED = {1: 1, 4: 4, 8: 8}
BOOL, BYTES32, BYTES64 = 16, 32, 64
NONE = 0xFFFFFFFF          # OXH_TAKE_NULL: an absent index; OXH_TAKE_NO_COLUMN: no fallback


class Taken(NamedTuple):
    """One output column: its kind and its buffers as uint8 arrays but the offsets (int32 / int64; None for
    the kinds without)."""
    kind: int
    nrows: int
    values: Any
    offsets: Any
    validity: Any


def bits(packed, bit0, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n].astype(bool)


def pack(mask):
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def index(a, n):
    """An index array as u32 (None: all absent; a signed array says absent with a negative value)."""
    if a is None:
        return np.full(n, NONE, dtype=np.uint32)
    a = np.asarray(a)
    if a.dtype.kind == "i":
        a = np.where(a < 0, NONE, a)
    return a.astype(np.uint32)


def valid_rows(col):
    return np.ones(col.nrows, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit, col.nrows)


def resolve(columns, idx, entry):
    """(source column, source row) of every output row; the source column is -1 for a null cell."""
    a, ia, b, ib = entry
    n = idx[0].size
    src = np.full(n, -1, dtype=np.int64)
    row = np.zeros(n, dtype=np.int64)
    for col, through in ((a, ia), (b, ib)):
        if col is None or col == NONE:
            continue
        r = idx[through].astype(np.int64)
        present = idx[through] != NONE
        assert (r[present] < columns[col].nrows).all(), "an index that is no row"
        ok = np.zeros(n, dtype=bool)
        ok[present] = valid_rows(columns[col])[r[present]]
        ok &= src < 0                       # the primary wins
        src[ok], row[ok] = col, r[ok]
    return src, row


def cell_spans(col):
    off = np.asarray(col.offsets).astype(np.int64)
    assert off.size == col.nrows + 1 and (np.diff(off) >= 0).all() and (col.nrows == 0 or off[0] >= 0)
    return off[:-1], off[1:] - off[:-1]


def take_one(columns, idx, entry):
    n = idx[0].size
    kind = columns[entry[0]].kind
    if entry[2] is not None and entry[2] != NONE:
        assert columns[entry[2]].kind == kind
    src, row = resolve(columns, idx, entry)
    validity = pack(src >= 0)
    used = [c for c in dict.fromkeys((entry[0], entry[2])) if c is not None and c != NONE]
    if kind in FIXED:
        w = FIXED[kind]
        out = np.zeros((n, w), dtype=np.uint8)
        for c in used:
            raw = np.ascontiguousarray(columns[c].values).view(np.uint8).reshape(-1)[:columns[c].nrows * w].reshape(-1, w)
            out[src == c] = raw[row[src == c]]
        return Taken(kind, n, out.reshape(-1), None, validity)
    if kind == BOOL:
        out = np.zeros(n, dtype=bool)
        for c in used:
            out[src == c] = bits(columns[c].values, columns[c].value_bit, columns[c].nrows)[row[src == c]]
        return Taken(kind, n, pack(out), None, validity)
    assert kind in (BYTES32, BYTES64), kind
    lens = np.zeros(n, dtype=np.int64)
    start = np.zeros(n, dtype=np.int64)
    for c in used:
        s, l = cell_spans(columns[c])
        lens[src == c], start[src == c] = l[row[src == c]], s[row[src == c]]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    values = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for c in used:
        mine = src == c
        l = lens[mine]
        total = int(l.sum())
        within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(l) - l, l)
        data = np.asarray(columns[c].values, dtype=np.uint8) if columns[c].values is not None else np.zeros(0, dtype=np.uint8)
        values[np.repeat(offsets[:-1][mine], l) + within] = data[np.repeat(start[mine], l) + within]
    if kind == BYTES32:
        assert offsets[-1] <= np.iinfo(np.int32).max
    return Taken(kind, n, values, offsets.astype(np.int32 if kind == BYTES32 else np.int64), validity)


def take(columns, idx0, idx1=None, plan=None):
    """The output columns of one call: a list of `Taken`. plan: (a, ia, b, ib) per output column, b None or
    NONE for no fallback; None = every column through idx0."""
    n = len(idx0) if idx0 is not None else len(idx1)
    idx = (index(idx0, n), index(idx1, n))
    if plan is None:
        plan = [(c, 0, None, 0) for c in range(len(columns))]
    return [take_one(columns, idx, tuple(entry)) for entry in plan]


def pylist(t, text=True):
    """The cells of a `Taken` (or a Column that starts at bit / offset 0) as Python values: None for a
    null, int for fixed width (the little-endian unsigned reading), bool, str / bytes."""
    valid = bits(t.validity, 0, t.nrows) if t.validity is not None else np.ones(t.nrows, dtype=bool)
    if t.kind in FIXED:
        raw = np.ascontiguousarray(t.values).view(np.uint8).reshape(t.nrows, FIXED[t.kind])
        cells = [int.from_bytes(r.tobytes(), "little") for r in raw]
    elif t.kind == BOOL:
        cells = bits(t.values, 0, t.nrows).tolist()
    else:
        data = np.asarray(t.values, dtype=np.uint8).tobytes()
        off = np.asarray(t.offsets).tolist()
        cells = [data[off[i]:off[i + 1]] for i in range(t.nrows)]
        if text:
            cells = [c.decode() for c in cells]
    return [c if v else None for c, v in zip(cells, valid.tolist())]
