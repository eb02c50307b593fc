"""The CPU restatement the concat tests compare with (tests/test_concat.py, test_concat_cpu.py): row ranges of
parts written one after the other, in plain numpy (`unpackbits`, slicing, `concatenate`), by the text of
include/oxen_hash.h. Columns are `oxen_amd.tabular.Column` descriptions over numpy arrays; nothing here calls
the library.

Output column c over N = sum(count) rows, buffers that start at bit / offset 0:
    validity     ceil(N / 8) bytes, LSB first, pad bits 0, a part without validity contributing ones
    fixed width  N * width bytes, as they are (under null cells too)
    boolean      ceil(N / 8) bytes, the bits as they are, pad bits 0
    bytes        N + 1 offsets of the column's own width from 0: the source offsets rebased; the bytes
                 [off[first], off[first + count]) of each part one after the other
"""
import numpy as np

from _take import BOOL, BYTES32, BYTES64, FIXED, Taken, bits, pack, valid_rows


def ranges_of(parts, ranges):
    return [(0, p[0].nrows) for p in parts] if ranges is None else [(int(f), int(n)) for f, n in ranges]


def rebased(off, base, device_reading):
    """(the part's output offsets, element `count` included; its span (lo, hi) in the source values).
    off: the count + 1 source offsets of the taken range."""
    lo, hi = int(off[0]), int(off[-1])
    if not device_reading:
        assert lo >= 0 and (np.diff(off) >= 0).all(), "offsets that are negative or decrease"
        return off - lo + base, (lo, hi)
    # the device form's reading of bad offsets: a span that is itself bad holds nothing; inside a good span the
    # offset after a bad pair is written as the offset before it, and every offset is clamped into the span
    if lo < 0 or hi < lo:
        return np.full(off.size, base, dtype=np.int64), (0, 0)
    v = off.copy()
    bad = (off[:-1] < 0) | (off[1:] < off[:-1])
    v[1:][bad] = off[:-1][bad]
    return base + np.clip(v, lo, hi) - lo, (lo, hi)


def has_bad_offsets(parts, ranges=None):
    for cols, (f, n) in zip(parts, ranges_of(parts, ranges)):
        for c in cols:
            if c.kind in (BYTES32, BYTES64) and n:
                off = np.asarray(c.offsets).astype(np.int64)[f:f + n + 1]
                if off[0] < 0 or (np.diff(off) < 0).any():
                    return True
    return False


def concat_one(parts, ranges, c, device_reading=False):
    kind = parts[0][c].kind
    taken = [(cols[c], f, n) for cols, (f, n) in zip(parts, ranges) if n]
    total = sum(n for _, _, n in taken)
    assert all(col.kind == kind for col, _, _ in taken)
    valid = [valid_rows(col)[f:f + n] for col, f, n in taken]
    validity = pack(np.concatenate(valid)) if valid else np.zeros(0, dtype=np.uint8)
    if kind in FIXED:
        w = FIXED[kind]
        raw = [np.ascontiguousarray(col.values).view(np.uint8).reshape(-1)[f * w:(f + n) * w] for col, f, n in taken]
        return Taken(kind, total, np.concatenate(raw) if raw else np.zeros(0, dtype=np.uint8), None, validity)
    if kind == BOOL:
        cells = [bits(col.values, col.value_bit, col.nrows)[f:f + n] for col, f, n in taken]
        return Taken(kind, total, pack(np.concatenate(cells)) if cells else np.zeros(0, dtype=np.uint8), None, validity)
    assert kind in (BYTES32, BYTES64), kind
    offsets, values, base = [], [], 0
    for k, (col, f, n) in enumerate(taken):
        off, (lo, hi) = rebased(np.asarray(col.offsets).astype(np.int64)[f:f + n + 1], base, device_reading)
        offsets.append(off if k + 1 == len(taken) else off[:-1])
        if hi > lo:
            values.append(np.asarray(col.values, dtype=np.uint8)[lo:hi])
        base += hi - lo
    offsets = np.concatenate(offsets) if offsets else np.zeros(1, dtype=np.int64)
    values = np.concatenate(values) if values else np.zeros(0, dtype=np.uint8)
    if kind == BYTES32:
        assert base <= np.iinfo(np.int32).max
    return Taken(kind, total, values, offsets.astype(np.int32 if kind == BYTES32 else np.int64), validity)


def concat(parts, ranges=None, device_reading=False):
    """The output columns of one call: a list of `Taken`. parts: a list of lists of Column; ranges: one
    (first, count) per part, None = whole parts. device_reading: the device form's reading of bad offsets."""
    parts = [list(p) for p in parts]
    ranges = ranges_of(parts, ranges)
    for cols, (f, n) in zip(parts, ranges):
        assert 0 <= f and 0 <= n and f + n <= cols[0].nrows
    return [concat_one(parts, ranges, c, device_reading) for c in range(len(parts[0]))]

