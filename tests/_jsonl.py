"""The JSON Lines rules of include/oxen_hash.h ("JSON Lines") restated in plain Python, sharing nothing with the
library: a sequential byte-by-byte state machine per line (the backslash run, the string state and the depth as
plain variables, not carries), the well-formed-record rule, the value kinds with int() / float() behind
re.fullmatch on the grammars and an unescape of its own, the names, the inference, and the Arrow buffers (packed
validity, offsets, values) with the per-column stats. Slow on purpose: the tests use it on small files and build
their large cases from known cells."""
import re
import struct
from typing import NamedTuple

import numpy as np

INT64, FLOAT64, BOOL, STRING, STRING64 = 1, 2, 3, 4, 5
TYPE_NAMES = {INT64: "Int64", FLOAT64: "Float64", BOOL: "Boolean", STRING: "String", STRING64: "LargeString"}
INT_OK, FLOAT_OK, BOOL_OK = 1, 2, 4
WS = b" \t\r"
NUMBER_RE = re.compile(rb"(-?)(0|[1-9][0-9]*)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?")
SIMPLE = {0x22: 0x22, 0x5C: 0x5C, 0x2F: 0x2F, 0x62: 8, 0x66: 12, 0x6E: 10, 0x72: 13, 0x74: 9}
HEX = b"0123456789abcdefABCDEF"
# the kind of a trimmed value slot
UNPARSABLE, STR, NESTED, TRUE, FALSE, NULL, INTEGER, NUMBER = range(8)


def lines_of(data: bytes) -> list:
    """The (start, end) of every line: the buffer splits at every newline; its end ends the last line."""
    spans, start = [], 0
    for at, c in enumerate(data):
        if c == 0x0A:
            spans.append((start, at))
            start = at + 1
    if start < len(data):
        spans.append((start, len(data)))
    return spans


def string_value(tok: bytes):
    """The unescaped bytes of a string token, or None where it is not one."""
    if len(tok) < 2 or tok[0] != 0x22 or tok[-1] != 0x22:
        return None
    inner, out, i = tok[1:-1], bytearray(), 0
    while i < len(inner):
        c = inner[i]
        if c == 0x22 or c < 0x20:
            return None
        if c != 0x5C:
            out.append(c)
            i += 1
            continue
        if i + 1 >= len(inner):
            return None
        e = inner[i + 1]
        if e in SIMPLE:
            out.append(SIMPLE[e])
            i += 2
            continue
        if e != 0x75:
            return None
        units = []
        for _ in range(2):
            h = inner[i + 2:i + 6]
            if len(h) != 4 or any(x not in HEX for x in h):
                return None
            units.append(int(h, 16))
            i += 6
            if not 0xD800 <= units[0] <= 0xDBFF or len(units) == 2:
                break
            if inner[i:i + 2] != b"\\u":
                return None
        if 0xDC00 <= units[0] <= 0xDFFF:
            return None
        if len(units) == 2:
            if not 0xDC00 <= units[1] <= 0xDFFF:
                return None
            cp = 0x10000 + ((units[0] - 0xD800) << 10) + (units[1] - 0xDC00)
        else:
            cp = units[0]
        out += chr(cp).encode("utf-8")
    return bytes(out)


def kind_of(slot: bytes) -> int:
    """The kind of a trimmed, non-empty value slot."""
    c = slot[:1]
    if c == b'"':
        return STR if string_value(slot) is not None else UNPARSABLE
    if c == b"{":
        return NESTED if len(slot) >= 2 and slot.endswith(b"}") else UNPARSABLE
    if c == b"[":
        return NESTED if len(slot) >= 2 and slot.endswith(b"]") else UNPARSABLE
    if slot == b"true":
        return TRUE
    if slot == b"false":
        return FALSE
    if slot == b"null":
        return NULL
    m = NUMBER_RE.fullmatch(slot)
    if m:
        return INTEGER if m.group(3) is None and m.group(4) is None else NUMBER
    return UNPARSABLE


def record_of(line: bytes):
    """None for a malformed record, else its fields in order: [(unescaped key, trimmed value slot)]."""
    body = line.strip(WS)
    if not body.startswith(b"{") or not body.endswith(b"}"):
        return None
    escaped = in_string = False
    depth, marks = 0, []          # the structural bytes at depth 1 outside strings, but the outer braces
    for at, c in enumerate(body):
        was_escaped, escaped = escaped, (c == 0x5C and not escaped)
        if c == 0x22 and not was_escaped:
            in_string = not in_string
            continue
        if in_string:
            continue
        if c in b"{[":
            if depth == 0 and at != 0:
                return None
            depth += 1
        elif c in b"}]":
            depth -= 1
            if depth <= 0 and at != len(body) - 1:
                return None               # the depth dips to 0 before the last byte
        elif c in b":," and depth == 1:
            marks.append(at)
    if in_string or depth != 0:
        return None
    if not marks:
        return [] if body[1:-1].strip(WS) == b"" else None
    if len(marks) % 2 == 0 or any(body[m] != (0x3A if k % 2 == 0 else 0x2C) for k, m in enumerate(marks)):
        return None
    edges = [0] + marks + [len(body) - 1]
    slots = [body[edges[k] + 1:edges[k + 1]].strip(WS) for k in range(len(edges) - 1)]
    fields = []
    for k in range(0, len(slots), 2):
        key = string_value(slots[k])
        if key is None or slots[k + 1] == b"":
            return None
        fields.append((key, slots[k + 1]))
    return fields


class Parsed(NamedTuple):
    stats8: tuple
    names: list       # the unescaped names (bytes)
    rows: list        # per row ncols cells: None (a missing key or a malformed record) or the trimmed value slot
    ncols: int
    window: int


def parse(data: bytes, infer_rows: int = 10000) -> Parsed:
    records, blank = [], 0
    for a, b in lines_of(data):
        line = data[a:b]
        if line.strip(WS) == b"":
            blank += 1
        else:
            records.append(record_of(line))
    names = []
    for fields in records[:infer_rows]:
        for key, _ in fields or []:
            if key not in names:
                names.append(key)
    rows, malformed, non_canonical, ignored, nested = [], 0, 0, 0, 0
    for fields in records:
        if fields is None:
            malformed += 1
            rows.append([None] * len(names))
            continue
        cells = {}
        for key, slot in fields:
            cells.setdefault(key, slot)        # the first occurrence wins
            ignored += key not in names
            nested += slot[:1] in (b"{", b"[")
        non_canonical += [key for key, _ in fields] != names[:len(fields)]
        rows.append([cells.get(name) for name in names])
    n = len(records)
    return Parsed((n, n, len(names), malformed, blank, non_canonical, ignored, nested), names, rows, len(names), min(infer_rows, n))


def float_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def parse_float(text: bytes):
    """(bits, deferred) of a number token: the correctly rounded double, and whether the device's exact path
    misses it (more than 19 significant digits, a mantissa above 2^53 or a decimal exponent outside +-22)."""
    m = NUMBER_RE.fullmatch(text)
    frac = m.group(3) or b""
    digits = (m.group(2) + frac).lstrip(b"0")
    exp = int(m.group(4) or 0) - len(frac)
    if not digits:
        deferred = False
    elif len(digits) > 19:
        deferred = True
    else:
        deferred = not (int(digits) <= 1 << 53 and abs(exp) <= 22)
    return float_bits(float(text)), deferred


def class_bits(slot) -> int:
    if slot is None:
        return INT_OK | FLOAT_OK | BOOL_OK
    kind = kind_of(slot)
    if kind == NULL:
        return INT_OK | FLOAT_OK | BOOL_OK
    if kind == INTEGER:
        return INT_OK | FLOAT_OK if -(1 << 63) <= int(slot) < 1 << 63 else FLOAT_OK
    return FLOAT_OK if kind == NUMBER else BOOL_OK if kind in (TRUE, FALSE) else 0


def infer(p: Parsed) -> list:
    types = []
    for c in range(p.ncols):
        bits, some = INT_OK | FLOAT_OK | BOOL_OK, False
        for row in p.rows[:p.window]:
            bits &= class_bits(row[c])
            some |= row[c] is not None and kind_of(row[c]) != NULL
        types.append(STRING if not some else INT64 if bits & INT_OK else FLOAT64 if bits & FLOAT_OK else BOOL if bits & BOOL_OK else STRING)
    return types


class Buffers(NamedTuple):
    values: np.ndarray     # int64 / uint64 bit patterns of the doubles / packed bits / bytes
    offsets: object        # int32 / int64 for a string column, else None
    validity: np.ndarray   # packed, LSB first, the bits past nrows zero
    stats4: tuple          # (null, null_unparsable, deferred, value_bytes)


def pack(mask) -> np.ndarray:
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def cell_value(slot, type_: int):
    """("null",) / ("bad",) / ("ok", value[, deferred]) of one cell as a type."""
    if slot is None:
        return ("null",)
    kind = kind_of(slot)
    if kind == NULL:
        return ("null",)
    if type_ in (STRING, STRING64):
        if kind == UNPARSABLE:
            return ("bad",)
        return ("ok", string_value(slot) if kind == STR else slot)
    if type_ == INT64:
        if kind == INTEGER and -(1 << 63) <= int(slot) < 1 << 63:
            return ("ok", int(slot))
        return ("bad",)
    if type_ == FLOAT64:
        return ("ok",) + parse_float(slot) if kind in (INTEGER, NUMBER) else ("bad",)
    return ("ok", kind == TRUE) if kind in (TRUE, FALSE) else ("bad",)


def column(p: Parsed, c: int, type_: int) -> Buffers:
    n = len(p.rows)
    got = [cell_value(row[c], type_) for row in p.rows]
    valid = [g[0] == "ok" for g in got]
    null, bad = sum(g[0] == "null" for g in got), sum(g[0] == "bad" for g in got)
    if type_ in (STRING, STRING64):
        chunks = [g[1] if g[0] == "ok" else b"" for g in got]
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(b) for b in chunks], out=offsets[1:])
        values = np.frombuffer(b"".join(chunks), dtype=np.uint8)
        return Buffers(values, offsets if type_ == STRING64 else offsets.astype(np.int32), pack(valid), (null, bad, 0, values.size))
    if type_ == BOOL:
        values = pack([g[0] == "ok" and g[1] for g in got])
        return Buffers(values, None, pack(valid), (null, bad, 0, values.size))
    words = np.zeros(n, dtype=np.uint64)
    for r, g in enumerate(got):
        if g[0] == "ok":
            words[r] = g[1] & 0xFFFFFFFFFFFFFFFF
    deferred = sum(g[2] for g in got if g[0] == "ok") if type_ == FLOAT64 else 0
    return Buffers(words, None, pack(valid), (null, bad, deferred, 8 * n))
