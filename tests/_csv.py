"""The CSV rules of include/oxen_hash.h ("CSV") restated in plain Python, sharing nothing with the library: a
sequential byte-by-byte tokenizer (a state machine, not the prefix-xor formulation), the field-value rule, the
typed parsers through int() / float() behind re.fullmatch on the grammars, the inference, and the Arrow buffers
(packed validity, offsets, values) with the per-column stats. Slow on purpose: the tests use it on small files
and build their large cases from known cells."""
import re
import struct
from typing import NamedTuple

import numpy as np

NO_QUOTE = 256
INT64, FLOAT64, BOOL, STRING, STRING64 = 1, 2, 3, 4, 5
TYPE_NAMES = {INT64: "Int64", FLOAT64: "Float64", BOOL: "Boolean", STRING: "String", STRING64: "LargeString"}
INT_OK, FLOAT_OK, BOOL_OK = 1, 2, 4

INT_RE = re.compile(rb"[+-]?[0-9]+")
FLOAT_RE = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")
SPECIAL_RE = re.compile(rb"([+-]?)(inf|infinity|nan)", re.IGNORECASE)
BOOL_RE = re.compile(rb"true|false", re.IGNORECASE)
QUIET_NAN = 0x7FF8000000000000


def tokenize(data: bytes, sep: int, quote: int):
    """([record], ended_inside): a record is the list of its fields' (start, end) spans of `data`."""
    records, fields, start, inside, ended = [], [], 0, False, True
    for at, c in enumerate(data):
        ended = False
        if c == quote:
            inside = not inside
        elif inside:
            pass
        elif c == sep:
            fields.append((start, at))
            start = at + 1
        elif c == 0x0A:
            fields.append((start, at))
            records.append(fields)
            fields, start, ended = [], at + 1, True
    if data and not ended:             # the end of the buffer ends the last record, whatever the parity
        fields.append((start, len(data)))
        records.append(fields)
    return records, inside


def field_value(raw: bytes, quote: int):
    """(value, quoted)."""
    if quote < NO_QUOTE and len(raw) >= 2 and raw[0] == quote and raw[-1] == quote:
        inner, out, k = raw[1:-1], bytearray(), 0
        while k < len(inner):
            out.append(inner[k])
            if inner[k] == quote and k + 1 < len(inner) and inner[k + 1] == quote:
                k += 1
            k += 1
        return bytes(out), True
    return raw, False


class Parsed(NamedTuple):
    stats8: tuple
    names: list       # the header's names (bytes); [] without a header
    rows: list        # per data row ncols cells: None (a missing field) or (value, quoted)
    ncols: int


def parse(data: bytes, sep: int = 0x2C, quote: int = 0x22, has_header: bool = True) -> Parsed:
    records, inside = tokenize(data, sep, quote)
    kept = []          # per kept record its fields' bytes, the '\r' off the record's own last field
    for fields in records:
        raws = [data[a:b] for a, b in fields]
        if raws[-1].endswith(b"\r"):
            raws[-1] = raws[-1][:-1]
        if raws != [b""]:
            kept.append(raws)
    ncols = len(kept[0]) if kept else 0
    names = [field_value(r, quote)[0] for r in kept[0]] if has_header and kept else []
    body = kept[1:] if has_header else kept
    short = sum(len(r) < ncols for r in body)
    long_ = sum(len(r) > ncols for r in body)
    rows = [[field_value(raws[c], quote) if c < len(raws) else None for c in range(ncols)] for raws in body]
    stats = (len(records), len(rows), ncols, sum(len(f) for f in records), len(records) - len(kept), short, long_, int(inside))
    return Parsed(stats, names, rows, ncols)


def float_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def parse_float(text: bytes):
    """None, or (bits, deferred): the correctly rounded double, and whether the device's exact path misses it."""
    m = SPECIAL_RE.fullmatch(text)
    if m:
        sign = 1 << 63 if m.group(1) == b"-" else 0
        return (QUIET_NAN if m.group(2).lower() == b"nan" else float_bits(float("inf"))) | sign, False
    m = FLOAT_RE.fullmatch(text)
    if not m:
        return None
    whole, frac = m.group(2) or b"", (m.group(3) if m.group(2) is not None else m.group(4)) or b""
    exp = int(m.group(5) or 0)
    digits = (whole + frac).lstrip(b"0")
    if not digits:
        deferred = False
    elif len(digits) > 19:
        deferred = True
    else:
        deferred = not (int(digits) <= 1 << 53 and abs(exp - len(frac)) <= 22)
    return float_bits(float(text)), deferred


def parse_int(text: bytes):
    """None (not the grammar), "range", or the value."""
    if not INT_RE.fullmatch(text):
        return None
    v = int(text)
    return v if -(1 << 63) <= v < 1 << 63 else "range"


def class_bits(value: bytes) -> int:
    if value == b"":
        return INT_OK | FLOAT_OK | BOOL_OK
    return ((INT_OK if isinstance(parse_int(value), int) else 0) | (FLOAT_OK if parse_float(value) is not None else 0) |
            (BOOL_OK if BOOL_RE.fullmatch(value) else 0))


def infer(p: Parsed, max_rows: int = 10000) -> list:
    types = []
    for c in range(p.ncols):
        bits, some = INT_OK | FLOAT_OK | BOOL_OK, False
        for row in p.rows[:max_rows]:
            cell = row[c]
            if cell is not None and cell[0] != b"":
                bits &= class_bits(cell[0])
                some = True
        types.append(STRING if not some else INT64 if bits & INT_OK else FLOAT64 if bits & FLOAT_OK else BOOL if bits & BOOL_OK else STRING)
    return types


class Buffers(NamedTuple):
    values: np.ndarray     # int64 / uint64 bit patterns of the doubles / packed bits / bytes
    offsets: object        # int32 / int64 for a string column, else None
    validity: np.ndarray   # packed, LSB first, the bits past nrows zero
    stats4: tuple          # (null_empty, null_unparsable, deferred, value_bytes)


def pack(mask) -> np.ndarray:
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def column(p: Parsed, c: int, type_: int) -> Buffers:
    n = len(p.rows)
    valid, empty, bad, deferred = [False] * n, 0, 0, 0
    if type_ in (STRING, STRING64):
        chunks = []
        for r, row in enumerate(p.rows):
            cell = row[c]
            if cell is None or (cell[0] == b"" and not cell[1]):
                empty += 1
                chunks.append(b"")
            else:
                valid[r] = True
                chunks.append(cell[0])
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(b) for b in chunks], out=offsets[1:])
        values = np.frombuffer(b"".join(chunks), dtype=np.uint8)
        return Buffers(values, offsets if type_ == STRING64 else offsets.astype(np.int32), pack(valid), (empty, 0, 0, values.size))
    words, truth = np.zeros(n, dtype=np.uint64), [False] * n
    for r, row in enumerate(p.rows):
        cell = row[c]
        if cell is None or cell[0] == b"":
            empty += 1
            continue
        text = cell[0]
        if type_ == INT64:
            v = parse_int(text)
            if isinstance(v, int):
                valid[r], words[r] = True, v & 0xFFFFFFFFFFFFFFFF
        elif type_ == FLOAT64:
            v = parse_float(text)
            if v is not None:
                valid[r], words[r] = True, v[0]
                deferred += v[1]
        else:
            if BOOL_RE.fullmatch(text):
                valid[r], truth[r] = True, text.lower() == b"true"
        bad += not valid[r]
    if type_ == BOOL:
        values = pack(truth)
        return Buffers(values, None, pack(valid), (empty, bad, 0, values.size))
    return Buffers(words, None, pack(valid), (empty, bad, deferred, 8 * n))


def cells_as_text(p: Parsed) -> list:
    """Per row the cells as bytes or None (null as a string column has it)."""
    return [[None if cell is None or (cell[0] == b"" and not cell[1]) else cell[0] for cell in row] for row in p.rows]
