"""The rules of include/oxen_hash.h "CSV text" restated in plain Python, sharing nothing with the library: the file is
built sequentially, cell by cell; a double's digits come from repr() (the shortest string that reads back, nearest
the value -- what ryu picks) and are laid out by ryu's five forms; a string is quoted when it must be. A frame here
is plain data: names (bytes), types, and per column a list of cells -- None for a null, an int, a float, a bool or
bytes. Slow on purpose: the tests use it on small frames and build their large cases from known cells."""
import math
from decimal import Decimal

INT64, FLOAT64, BOOL, STRING, STRING64 = 1, 2, 3, 4, 5
MIN_NORMAL = 2.2250738585072014e-308


def float_digits(a: float):
    """(d, k): the shortest digits of a finite a > 0 as a string without trailing zeros, a = d x 10^k."""
    _, digits, k = Decimal(repr(a)).as_tuple()
    d = "".join(map(str, digits)).lstrip("0")
    stripped = d.rstrip("0")
    return stripped, k + len(d) - len(stripped)


def float_text(x: float) -> bytes:
    if math.isnan(x):
        return b"NaN"
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    if math.isinf(x):
        return (sign + "inf").encode()
    if x == 0.0:
        return (sign + "0.0").encode()
    d, k = float_digits(abs(x))
    n = len(d)
    kk = n + k
    if 0 <= k and kk <= 16:
        text = d + "0" * k + ".0"
    elif 0 < kk <= 16:
        text = d[:kk] + "." + d[kk:]
    elif -5 < kk <= 0:
        text = "0." + "0" * -kk + d
    elif n == 1:
        text = f"{d}e{kk - 1}"
    else:
        text = f"{d[0]}.{d[1:]}e{kk - 1}"
    return (sign + text).encode()


def float_deferred(x: float) -> bool:
    """Outside the exact path's stated domain: a finite non-zero double that is subnormal, or 1e15 and above, or has
    16 or 17 shortest digits, or digits further than 22 places behind the point."""
    if math.isnan(x) or math.isinf(x) or x == 0.0:
        return False
    a = abs(x)
    if a < MIN_NORMAL or a >= 1e15:
        return True
    d, k = float_digits(a)
    return len(d) > 15 or -k > 22


def string_text(raw: bytes, sep: int, quote: int):
    """(text, quoted): quote style "necessary"."""
    if len(raw) == 0 or any(c in (sep, quote, 0x0A, 0x0D) for c in raw):
        q = bytes([quote])
        return q + raw.replace(q, q + q) + q, True
    return raw, False


def cell_text(t: int, v, sep: int, quote: int):
    """(text, quoted, deferred) of one present cell."""
    if t == INT64:
        return str(int(v)).encode(), False, False
    if t == BOOL:
        return (b"true" if v else b"false"), False, False
    if t == FLOAT64:
        return float_text(float(v)), False, float_deferred(float(v))
    text, quoted = string_text(bytes(v), sep, quote)
    return text, quoted, False


def write(names, types, columns, sep=0x2C, quote=0x22, header=True):
    """(the file's bytes, stats4 = (bytes, quoted cells with the header's, deferred float cells, null cells))."""
    out = bytearray()
    quoted_cells = deferred_cells = nulls = 0
    sep_byte = bytes([sep])
    if header:
        fields = []
        for name in names:
            text, quoted = string_text(bytes(name), sep, quote)
            quoted_cells += quoted
            fields.append(text)
        out += sep_byte.join(fields) + b"\n"
    nrows = len(columns[0]) if columns else 0
    for r in range(nrows):
        for c, column in enumerate(columns):
            if c:
                out += sep_byte
            v = column[r]
            if v is None:
                nulls += 1
                continue
            text, quoted, deferred = cell_text(types[c], v, sep, quote)
            quoted_cells += quoted
            deferred_cells += deferred
            out += text
        out += b"\n"
    return bytes(out), (len(out), quoted_cells, deferred_cells, nulls)
