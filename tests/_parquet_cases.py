"""The cells of the Parquet reader's fixtures (tests/golden/parquet/*.parquet) as one function of the row number:
tests/golden/make_df_parquet.py writes them with pyarrow, tests/test_parquet_read*.py expect them. Stretches of a
hundred rows without a null give RLE level runs beside the bit-packed ones. Also the helpers those tests share."""
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet")
ROWS = 900
FILES = ("v1_dict_fallback", "v2_dict_fallback", "v2_plain")
# name, numpy dtype of a fixed-width column ("bool" / "str" otherwise), REQUIRED
COLUMNS = (("i64", "<i8", False), ("i32", "<i4", False), ("f32", "<f4", False), ("b", "bool", False), ("f64", "<f8", False),
           ("s", "str", False), ("u", "str", False), ("req", "<i8", True), ("nul", "<i8", False))
_F64 = (0.5, float("nan"), -0.0, float("inf"), float("-inf"), 0.0, -2.5e300, 5e-324)
_S = ("", "a", "é", "日本語", "plain ascii text", "tab\there", "🦬 ox", "x" * 40)


def cells(n: int) -> dict:
    quiet = lambda r: (r // 100) % 4 == 1   # noqa: E731  rows 100-199, 500-599: no nulls, whole pages of one RLE run
    null = lambda r, m, k: r % m == k and not quiet(r)   # noqa: E731
    return {
        "i64": [None if null(r, 11, 3) else (r * 7919 % 17) * 1000003 - (1 << 40) for r in range(n)],          # 17 distinct values
        "i32": [None if null(r, 7, 5) else (r * 2654435761 % (1 << 32)) - (1 << 31) for r in range(n)],       # all distinct
        "f32": [struct.unpack("<f", struct.pack("<f", (0.5, -1.25, 3e38)[r % 3]))[0] for r in range(n)],      # 3 distinct, no nulls
        "b": [None if null(r, 5, 4) else (r < 300 or (r * r + r // 3) % 3 == 0) for r in range(n)],           # long runs, then mixed
        "f64": [None if null(r, 9, 1) else (_F64[r % 8] if r % 3 else r * 0.125) for r in range(n)],
        "s": [None if null(r, 6, 2) else _S[r * 31 % 37 % 8] + ("" if r % 37 else "!" * (r % 5)) for r in range(n)],
        "u": ["row-%05d-%s" % (r, "x" * (r % 23)) for r in range(n)],                                        # all distinct
        "req": [r * 3 - 1000 for r in range(n)],
        "nul": [None] * n,
    }


# unsupported.parquet: a FIXED_LEN_BYTE_ARRAY column between an INT64 and a DATE (int32 days), pyarrow's defaults
UNSUPPORTED_ROWS = 300


def unsupported_cells(n: int) -> dict:
    ints = [None if r % 4 == 1 else r - 50 for r in range(n)]
    return {"a": ints, "fixed": [b"%04d" % r for r in range(n)], "d": ints}


# many_pages.parquet: 60 000 rows in DataPage V2 pages of 100 rows, dictionary-coded: 600 pages a column
MANY_ROWS = 60000
MANY_COLUMNS = (("i64", "<i8", False), ("s", "str", False), ("b", "bool", False))


def many_cells(n: int) -> dict:
    whole = cells(ROWS)
    return {name: [whole[name][(r * 7 + r // ROWS) % ROWS] for r in range(n)] for name, _, _ in MANY_COLUMNS}


def expected(name: str, dtype: str, column: list):
    """(validity as booleans, values, offsets) as a reader must give them: a null's slot is 0 / false / no bytes;
    values are a numpy array of the dtype's unsigned bits, booleans, or the strings' bytes."""
    valid = np.array([c is not None for c in column], dtype=bool)
    if dtype == "str":
        raw = [b"" if c is None else c.encode("utf-8") for c in column]
        return valid, np.frombuffer(b"".join(raw), dtype=np.uint8), np.cumsum([0] + [len(b) for b in raw])
    if dtype == "bool":
        return valid, np.array([bool(c) for c in column], dtype=bool), None
    filled = [0 if c is None else c for c in column]
    return valid, np.array(filled, dtype=dtype).view("<u" + dtype[2]), None


# ---------------------------------------------------------------- what the reader's tests share
def fixture_bytes(name: str) -> bytes:
    with open(os.path.join(GOLDEN, name + ".parquet"), "rb") as f:
        return f.read()


def wanted(columns, column_cells: dict) -> dict:
    """{name: (kind, validity, values, offsets)} of a fixture's cells, in `parts`' form."""
    from oxen_amd import _capi

    kind = {"bool": _capi.OXH_COL_BOOL, "str": _capi.OXH_COL_BYTES32, "<i4": 4, "<f4": 4, "<i8": 8, "<f8": 8}
    return {name: (kind[dtype],) + expected(name, dtype, column_cells[name]) for name, dtype, _ in columns}


def to_host(col):
    down = lambda t: None if t is None else (np.asarray(t) if isinstance(t, np.ndarray) else t.cpu().numpy())  # noqa: E731
    return col._replace(values=down(col.values), offsets=down(col.offsets), validity=down(col.validity))


def parts(col):
    """(kind, validity as booleans, values with the nulls' slots as they are, offsets) of a host Column."""
    from oxen_amd import _capi

    n = col.nrows
    bits = lambda a, at: np.unpackbits(np.asarray(a, dtype=np.uint8), bitorder="little")[at:at + n].astype(bool)  # noqa: E731
    valid = np.ones(n, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit)
    if col.kind == _capi.OXH_COL_BOOL:
        return col.kind, valid, bits(col.values, col.value_bit), None
    if col.kind in (_capi.OXH_COL_FIXED4, _capi.OXH_COL_FIXED8):
        return col.kind, valid, np.ascontiguousarray(col.values).view("<u%d" % col.kind), None
    offsets = np.asarray(col.offsets).astype(np.int64)
    return col.kind, valid, np.asarray(col.values)[int(offsets[0]):int(offsets[-1])], offsets - offsets[0]


def assert_same(got, want, name):
    """Bit for bit: the kind, the validity, the offsets, the values -- a null's slot read back as 0 / false / no bytes.
    want: a host Column, or `parts`' tuple."""
    gk, gvalid, gvalues, goffsets = parts(to_host(got))
    wk, wvalid, wvalues, woffsets = want if type(want) is tuple else parts(want)
    assert gk == wk and np.array_equal(gvalid, wvalid), name
    if goffsets is None:
        assert np.array_equal(gvalues, np.where(wvalid, wvalues, 0)), name
        assert got.validity is not None and not np.any(np.unpackbits(to_host(got).validity, bitorder="little")[got.nrows:]), name
    else:   # the frame's null strings may hold bytes; the reader's hold none
        lens = np.where(wvalid, np.diff(woffsets), 0)
        keep = np.repeat(wvalid, np.diff(woffsets))   # the bytes of the cells that are not null
        assert np.array_equal(goffsets, np.concatenate([[0], np.cumsum(lens)])) and gvalues.tobytes() == np.asarray(wvalues)[keep].tobytes(), name
