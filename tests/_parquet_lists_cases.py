"""The cells of the Parquet reader's list fixtures (tests/golden/parquet/lists_*.parquet) as one function of the row
number: tests/golden/make_df_parquet_lists.py writes them with pyarrow, tests/test_parquet_lists*.py expect them as
plain Python lists turned into Arrow's four buffers."""
import struct

import numpy as np

ROWS = 900
LONG_ROW, LONG = 450, 300   # one row that crosses 64-entry words and pages
FILES = ("lists_v1", "lists_v2", "lists_v1_snappy", "lists_v2_zstd")
# name, numpy dtype of the elements, nullable list, nullable elements, fixed size (0: none)
LISTS = (("li64", "<i8", True, True, 0), ("lf32", "<f4", True, False, 0), ("emb", "<f4", False, False, 8), ("li32", "<i4", True, True, 0),
         ("lf64", "<f8", True, True, 0))
FLAT = ("i", "s")
DIM = 8


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _li64(r):
    if (r // 100) % 4 == 1:   # rows 100-199, 500-599: one element, not null: both level streams are single RLE runs
        return [r * 3 - 1000]
    if r == LONG_ROW:
        return [(r + j) * 1000003 - (1 << 40) for j in range(LONG)]
    if r % 13 == 4:
        return None
    return [None if (r + j) % 5 == 0 else (r * 7919 + j) * 1000003 - (1 << 40) for j in range(r % 6)]


def cells(n: int) -> dict:
    return {
        "li64": [_li64(r) for r in range(n)],
        "lf32": [None if r % 17 == 3 else [_f32((r * 4 + j) * 0.25 - 100) for j in range(r % 4)] for r in range(n)],
        "emb": [[float((r * DIM + j) * 37 % 17 - 8) for j in range(DIM)] for r in range(n)],   # integers up to 8: sums exact in any order
        "li32": [None if r % 19 == 7 else [None if (r + j) % 11 == 0 else (r + j) % 5 * 1000 - 2000 for j in range(r % 3 + 1)] for r in range(n)],   # 5 distinct: a dictionary
        "lf64": [None if r % 23 == 5 else [None if (r * 3 + j) % 7 == 0 else r + j / 8.0 for j in range(r % 5)] for r in range(n)],                  # all distinct
        "i": [None if r % 11 == 3 else r * 3 - 1000 for r in range(n)],
        "s": [None if r % 6 == 2 else "row-%d" % r for r in range(n)],
    }


# lists_split_rows.parquet: one list<int64> column whose pages are cut every SPLIT_PAGE level entries, wherever a row is
SPLIT_ROWS, SPLIT_PAGE = 120, 37


def split_cells(n: int) -> list:
    def cell(r):
        if r % 7 == 3:
            return None
        if r % 5 == 0:
            return []
        return [None if (r + j) % 4 == 0 else r * 1000 + j for j in range(100 if r == 41 else r % 9 + 1)]   # row 41 spans pages that start no row
    return [cell(r) for r in range(n)]


def expected(dtype: str, column: list):
    """(offsets, the lists' validity, the elements' validity, the elements' unsigned bits) as a reader must give
    them: a null list has no elements, a null element's value is 0."""
    offsets, valid, child, values = [0], [], [], []
    for cell in column:
        valid.append(cell is not None)
        for e in cell or []:
            child.append(e is not None)
            values.append(0 if e is None else e)
        offsets.append(len(values))
    return (np.array(offsets, dtype=np.int64), np.array(valid, dtype=bool), np.array(child, dtype=bool),
            np.array(values, dtype=dtype).view("<u" + dtype[2]))


def bits(bitmap, n):
    return np.unpackbits(np.asarray(bitmap, dtype=np.uint8), bitorder="little")[:n].astype(bool)
