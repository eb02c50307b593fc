"""The CPU restatement the filter tests compare with (tests/test_filter_rows.py, test_filter_rows_cpu.py): the
semantics of include/oxen_hash.h ("row filter") in plain Python, row by row. Columns are
`oxen_amd.tabular.Column` descriptions over numpy arrays; terms and logical operators come in the ABI's form
(what `oxen_amd.tabular.filter_terms` returns). Nothing here calls the library, and neither polars nor pyarrow
is needed.

A cell is None for a null, else a Python value whose own comparison is the column's order: an int for signed /
unsigned cells and booleans (false 0 < true 1), `bytes` for a byte cell (Python compares them unsigned byte-wise,
a proper prefix first; b"" is a value), and for OXH_SORT_FLOAT the pair (0, v) with -0.0 as 0.0, or (1, 0.0) for
every NaN: numeric order, the zeros equal, the NaNs equal and above +inf. A term on None is None; && and || are
Kleene's over True / False / None; the terms are folded left to right with no precedence; a row is selected
exactly when the fold is True.
"""
import math
import operator
import struct

import numpy as np

FIXED = {1: 1, 4: 4, 8: 8}
BOOL, BYTES32, BYTES64 = 16, 32, 64
SIGNED, UNSIGNED, FLOAT = 0, 1, 2
EQ, NE, LT, LE, GT, GE = range(6)
AND, OR = 0, 1
OPS = {EQ: operator.eq, NE: operator.ne, LT: operator.lt, LE: operator.le, GT: operator.gt, GE: operator.ge}
OP_NAMES = {"==": EQ, "!=": NE, "<": LT, "<=": LE, ">": GT, ">=": GE}


def bits(packed, bit0, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n].astype(bool)


def float_key(v):
    return (1, 0.0) if math.isnan(v) else (0, v + 0.0)   # -0.0 + 0.0 is +0.0


def fixed_value(raw, width, order):
    """The comparable value of `width` little-endian bytes given as an unsigned int."""
    raw &= (1 << (8 * width)) - 1
    if order == FLOAT:
        assert width in (4, 8)
        return float_key(struct.unpack("<f" if width == 4 else "<d", raw.to_bytes(width, "little"))[0])
    if order == SIGNED and raw >> (8 * width - 1):
        return raw - (1 << (8 * width))
    return raw


def cells(col, order=SIGNED, empty=()):
    """One comparable value per row, None for a null. empty: rows whose byte cell counts as b"" whatever its
    offsets say (what the device form makes of a bad pair of offsets)."""
    n = col.nrows
    valid = np.ones(n, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit, n)
    if col.kind in FIXED:
        w = FIXED[col.kind]
        raw = np.ascontiguousarray(col.values).view(np.uint8).reshape(-1)[:n * w]
        values = [fixed_value(v, w, order) for v in raw.view({1: np.uint8, 4: "<u4", 8: "<u8"}[w]).tolist()]
    elif col.kind == BOOL:
        values = [int(v) for v in bits(col.values, col.value_bit, n).tolist()]
    else:
        assert col.kind in (BYTES32, BYTES64)
        off = np.asarray(col.offsets).astype(np.int64).tolist()
        data = np.asarray(col.values, dtype=np.uint8).tobytes() if col.values is not None else b""
        values = [b"" if i in empty else data[off[i]:off[i + 1]] for i in range(n)]
    return [v if ok else None for v, ok in zip(values, valid.tolist())]


def literal(col, order, lit):
    """The term's literal (an int word, or bytes) as a value of the column's kind."""
    if col.kind in FIXED:
        return fixed_value(int(lit), FIXED[col.kind], order)
    if col.kind == BOOL:
        assert lit in (0, 1)
        return int(lit)
    return bytes(lit)


def and3(a, b):
    if a is False or b is False:
        return False
    return None if a is None or b is None else True


def or3(a, b):
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


def fold(results, logical):
    """Left to right, no precedence: a || b && c is (a || b) && c."""
    sofar = results[0]
    for r, op in zip(results[1:], logical):
        sofar = or3(sofar, r) if op == OR else and3(sofar, r)
    return sofar


def row_results(columns, terms, logical, orders=None, empty=None):
    """True / False / None per row."""
    orders = [SIGNED] * len(columns) if orders is None else list(orders)
    empty = empty or {}
    assert len(terms) >= 1 and len(logical) == len(terms) - 1
    per_term = []
    for c, op, lit in terms:
        want = literal(columns[c], orders[c], lit)
        per_term.append([None if v is None else bool(OPS[op](v, want)) for v in cells(columns[c], orders[c], empty.get(c, ()))])
    return [fold(list(r), logical) for r in zip(*per_term)]


class Selection:
    def __init__(self, idx, mask, stats, results):
        self.idx, self.mask, self.stats, self.results = idx, mask, stats, results


def filter_rows(columns, terms, logical=(), orders=None, empty=None):
    """idx (uint32, the selected rows ascending), mask (uint8: 8 * ceil(n / 64) bytes, LSB first, tail bits 0) and
    the two stats (selected, rows whose result is null)."""
    results = row_results(columns, terms, list(logical), orders, empty)
    picked = np.array([r is True for r in results], dtype=bool)
    mask = np.zeros(8 * -(-len(results) // 64), dtype=np.uint8)
    packed = np.packbits(picked, bitorder="little")
    mask[:packed.size] = packed
    stats = (int(picked.sum()), sum(1 for r in results if r is None))
    return Selection(np.nonzero(picked)[0].astype(np.uint32), mask, stats, results)
