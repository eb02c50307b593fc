"""The CPU restatement the row-sort tests compare with (tests/test_sort_rows.py, test_sort_rows_cpu.py): the
order of include/oxen_hash.h ("stable multi-column row sort") as Python's stable `sorted` over the row
indices with a tuple key per row. Columns are `oxen_amd.tabular.Column` descriptions over numpy arrays;
nothing here calls the library, and neither polars nor pyarrow is needed.

One key column gives one entry of a row's key: (0,) for a null, else (1, canonical value) -- the integer a
signed or unsigned cell holds; for a float (1, 0, value) with -0.0 folded into 0.0 and (1, 1) for every NaN, so
that all NaNs are equal and above +inf; False / True; the cell's `bytes`, which Python compares as unsigned
bytes with a proper prefix first. Tuples compare entry by entry, `sorted` is stable: rows equal on every key
keep their input order.
"""
import math
from collections import Counter

import numpy as np

FIXED = {1: 1, 4: 4, 8: 8}
BOOL, BYTES32, BYTES64 = 16, 32, 64
SIGNED, UNSIGNED, FLOAT = 0, 1, 2


def bits(packed, bit0, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n].astype(bool)


def cells(col, order=SIGNED):
    """The key entries of one column, one per row."""
    n = col.nrows
    valid = np.ones(n, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit, n)
    if col.kind in FIXED:
        w = FIXED[col.kind]
        raw = np.ascontiguousarray(col.values).view(np.uint8).reshape(-1)[:n * w]
        if order == FLOAT:
            assert w in (4, 8)
            out = []
            for v in raw.view(np.float32 if w == 4 else np.float64).tolist():
                out.append((1, 1) if math.isnan(v) else (1, 0, v + 0.0 if v != 0 else 0.0))
            values = out
        else:
            dt = {(1, SIGNED): np.int8, (4, SIGNED): np.int32, (8, SIGNED): np.int64,
                  (1, UNSIGNED): np.uint8, (4, UNSIGNED): np.uint32, (8, UNSIGNED): np.uint64}[w, order]
            values = [(1, v) for v in raw.view(dt).tolist()]
    elif col.kind == BOOL:
        values = [(1, v) for v in bits(col.values, col.value_bit, n).tolist()]
    else:
        assert col.kind in (BYTES32, BYTES64)
        off = np.asarray(col.offsets).astype(np.int64).tolist()
        data = np.asarray(col.values, dtype=np.uint8).tobytes() if col.values is not None else b""
        values = [(1, data[off[i]:off[i + 1]]) for i in range(n)]
    return [v if ok else (0,) for v, ok in zip(values, valid.tolist())]


def row_keys(columns, orders=None):
    orders = [SIGNED] * len(columns) if orders is None else list(orders)
    per_column = [cells(c, o) for c, o in zip(columns, orders)]
    return list(zip(*per_column)) if per_column else []


def sort_indices(columns, orders=None):
    """(perm, tied): perm[i] (uint32) = the row at place i of the sorted frame; tied = the rows that equal
    another row on every key (stats3[2])."""
    keys = row_keys(columns, orders)
    perm = sorted(range(len(keys)), key=keys.__getitem__)
    seen = Counter(keys)
    tied = sum(c for c in seen.values() if c > 1)
    return np.array(perm, dtype=np.uint32), tied


def byte_rounds(cells_of_group):
    """The refinement rounds a group of present byte cells tied so far needs in one column: chunks of 8 bytes
    are compared until no two cells still agree and still have bytes left. Returns the rounds this column
    takes while ties last (at least 1)."""
    alive, chunk = list(cells_of_group), 0
    while True:
        chunk += 1
        groups = Counter((c[:8 * chunk], len(c) >= 8 * chunk) for c in alive)
        alive = [c for c in alive if groups[(c[:8 * chunk], len(c) >= 8 * chunk)] > 1 and len(c) >= 8 * chunk]
        if not alive:
            return chunk
