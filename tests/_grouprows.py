"""The CPU restatement the grouping tests compare with (tests/test_group_rows.py, test_group_rows_cpu.py): the
equality of include/oxen_hash.h ("rows grouped by equality") as a plain Python dict over one tuple per row, in
row order. Columns are `oxen_amd.tabular.Column` descriptions over numpy arrays; nothing here calls the
library, and neither polars nor pyarrow is needed.

One key column gives one entry of a row's key: None for a null; the cell's `bytes` for a byte cell ("" is
b"", not None); for OXH_SORT_FLOAT the float 0.0 for both zeros and the string "nan" for every NaN, else the
float; otherwise -- fixed-width cells of the other classes, booleans -- the integer of the cell's bytes. Tuples
compare position by position, and a position holds one column's entries only.
"""
import math

import numpy as np

FIXED = {1: 1, 4: 4, 8: 8}
BOOL, BYTES32, BYTES64 = 16, 32, 64
SIGNED, UNSIGNED, FLOAT = 0, 1, 2
NAN = "nan"   # the one value every NaN is


def bits(packed, bit0, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n].astype(bool)


def strings(cells, kind=BYTES32, valid=None, bit=0, lead=b""):
    """A byte column from a list of bytes: `lead` bytes before the first cell (so offsets[0] != 0), the
    validity bitmap's row 0 at `bit`. A null cell keeps its bytes underneath, as Arrow allows."""
    import _rowhash
    from oxen_amd.tabular import Column

    off = np.zeros(len(cells) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cells], out=off[1:])
    data = np.frombuffer(lead + b"".join(cells), dtype=np.uint8)
    offsets = (off + len(lead)).astype(np.int32 if kind == BYTES32 else np.int64)
    return Column(kind, len(cells), data, offsets, None if valid is None else _rowhash.packed_at(valid, bit), 0,
                  0 if valid is None else bit)


def cells(col, order=SIGNED, empty=()):
    """The key entries of one column, one per row. empty: rows whose byte cell counts as b"" whatever its
    offsets say (what the device form makes of a bad pair of offsets)."""
    n = col.nrows
    valid = np.ones(n, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit, n)
    if col.kind in FIXED:
        w = FIXED[col.kind]
        raw = np.ascontiguousarray(col.values).view(np.uint8).reshape(-1)[:n * w]
        if order == FLOAT:
            assert w in (4, 8)
            values = [NAN if math.isnan(v) else (0.0 if v == 0 else v) for v in raw.view(np.float32 if w == 4 else np.float64).tolist()]
        else:
            values = raw.view({1: np.uint8, 4: "<u4", 8: "<u8"}[w]).tolist()   # the integer of the cell's bytes
    elif col.kind == BOOL:
        values = [int(v) for v in bits(col.values, col.value_bit, n).tolist()]
    else:
        assert col.kind in (BYTES32, BYTES64)
        off = np.asarray(col.offsets).astype(np.int64).tolist()
        data = np.asarray(col.values, dtype=np.uint8).tobytes() if col.values is not None else b""
        values = [b"" if i in empty else data[off[i]:off[i + 1]] for i in range(n)]
    return [v if ok else None for v, ok in zip(values, valid.tolist())]


def row_keys(columns, orders=None, empty=None):
    orders = [SIGNED] * len(columns) if orders is None else list(orders)
    empty = empty or {}
    per_column = [cells(c, o, empty.get(k, ())) for k, (c, o) in enumerate(zip(columns, orders))]
    return list(zip(*per_column)) if per_column else []


def encoded_length(columns, key):
    """The bytes of a row's key image: a tag per cell, the cell, a byte cell's length in the width of the
    column's offsets. Only `long_rows` depends on it."""
    total = 0
    for c, v in zip(columns, key):
        total += 1
        if v is None:
            continue
        total += FIXED[c.kind] if c.kind in FIXED else 1 if c.kind == BOOL else (4 if c.kind == BYTES32 else 8) + len(v)
    return total


class Groups:
    def __init__(self, group, count, first_idx, first_count, stats):
        self.group, self.count, self.first_idx, self.first_count, self.stats = group, count, first_idx, first_count, stats


def group_rows(columns, orders=None, empty=None):
    """group, count, first_idx, first_count (uint32) and the four stats (groups, duplicated, largest, long rows)."""
    keys = row_keys(columns, orders, empty)
    first = {}
    group = []
    for i, k in enumerate(keys):
        group.append(first.setdefault(k, i))
    sizes = {}
    for g in group:
        sizes[g] = sizes.get(g, 0) + 1
    count = [sizes[g] for g in group]
    first_idx = [i for i, g in enumerate(group) if g == i]
    first_count = [sizes[i] for i in first_idx]
    long_rows = sum(1 for k in keys if encoded_length(columns, k) > 240)
    stats = (len(first_idx), sum(1 for c in count if c > 1), max(count, default=0), long_rows)
    as_u32 = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
    return Groups(as_u32(group), as_u32(count), as_u32(first_idx), as_u32(first_count), stats)
