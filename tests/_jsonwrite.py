"""The rules of include/oxen_hash.h "JSON text" restated in plain Python, sharing nothing with the library: the file is
built sequentially, cell by cell, in both formats; a string is escaped byte by byte from a table written out here; a
finite double's text is tests/_csvwrite.py's (repr() behind the digits, ryu's five forms), taken by import as the
rules say it is the same text. A frame is plain data as in tests/_csvwrite.py: names (bytes), types, and per column a
list of cells -- None for a null, an int, a float, a bool or bytes. Slow on purpose."""
import importlib.util
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


_W = _load("_csvwrite_restatement", os.path.join(HERE, "_csvwrite.py"))
float_text, float_deferred = _W.float_text, _W.float_deferred
INT64, FLOAT64, BOOL, STRING, STRING64 = 1, 2, 3, 4, 5
LINES, ARRAY = 0, 1

SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def byte_text(c: int) -> bytes:
    if c in SHORT:
        return SHORT[c]
    if c < 0x20:
        return b"\\u00" + b"0123456789abcdef"[c >> 4:(c >> 4) + 1] + b"0123456789abcdef"[c & 15:(c & 15) + 1]
    return bytes([c])


def string_text(raw: bytes):
    """(text, escaped): the quotes, every byte by the table; escaped iff at least one byte widened."""
    body = b"".join(byte_text(c) for c in raw)
    return b'"' + body + b'"', len(body) != len(raw)


def cell_text(t: int, v):
    """(text, escaped, deferred, null) of one cell."""
    if v is None:
        return b"null", False, False, True
    if t == INT64:
        return str(int(v)).encode(), False, False, False
    if t == BOOL:
        return (b"true" if v else b"false"), False, False, False
    if t == FLOAT64:
        x = float(v)
        if math.isnan(x) or math.isinf(x):
            return b"null", False, False, True
        return float_text(x), False, float_deferred(x), False
    text, escaped = string_text(bytes(v))
    return text, escaped, False, False


def write(names, types, columns, fmt=LINES):
    """(the file's bytes, stats4 = (bytes, escaped string cells -- a name that needs escaping once, when there are
    rows --, deferred float cells, cells written as null))."""
    nrows = len(columns[0]) if columns else 0
    escaped_cells = deferred_cells = nulls = 0
    keys = []
    for name in names:
        text, escaped = string_text(bytes(name))
        escaped_cells += escaped and nrows > 0
        keys.append(text + b":")
    rows = []
    for r in range(nrows):
        fields = []
        for c, column in enumerate(columns):
            text, escaped, deferred, null = cell_text(types[c], column[r])
            escaped_cells += escaped
            deferred_cells += deferred
            nulls += null
            fields.append(keys[c] + text)
        rows.append(b"{" + b",".join(fields) + b"}")
    out = b"[" + b",".join(rows) + b"]" if fmt == ARRAY else b"".join(row + b"\n" for row in rows)
    return out, (len(out), escaped_cells, deferred_cells, nulls)
