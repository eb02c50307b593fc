"""Array restatements and input generators for the tabular tests past the grid caps
(tests/test_tabular_past_grid.py, pinned by tests/test_tabular_arrays_cpu.py).

The plain-Python restatements (`_keyeddiff.keyed_diff`, `_sortrows.sort_indices`,
`_rowhash.compute_new_row_indices`) stay the statement of record; at millions of rows they take too long, so
each has a numpy-only form here, restricted to the inputs the big cases use, and the CPU test pins every one
of them to its original with exact equality. Columns are `oxen_amd.tabular.Column` descriptions over numpy
arrays; nothing here calls the library.

The generators take the edge they plant rows around (the rows of one full launch of the capped grid, or the
elements of one full launch of the scan) as an argument, so the CPU test can check the planted structure at
a small edge.
"""
import numpy as np

from oxen_amd.tabular import Column

FIXED = {1: 1, 4: 4, 8: 8}
BOOL, BYTES32, BYTES64 = 16, 32, 64
SIGNED, UNSIGNED = 0, 1
UNCHANGED, ADDED, REMOVED, MODIFIED = 0, 1, 2, 3
NONE = 0xFFFFFFFF


def bits(packed, bit0, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n].astype(bool)


def packed_at(mask, bit0, rng):
    """An LSB-first bitmap that holds `mask` from bit `bit0` on; the bits before and after are noise."""
    mask = np.asarray(mask, dtype=bool)
    lead = rng.integers(0, 2, size=bit0).astype(bool)
    tail = rng.integers(0, 2, size=(-(bit0 + mask.size)) % 8).astype(bool)
    return np.packbits(np.concatenate([lead, mask, tail]), bitorder="little")


# ---------------------------------------------------------------- restatements
def valid_rows(col):
    return np.ones(col.nrows, dtype=bool) if col.validity is None else bits(col.validity, col.validity_bit, col.nrows)


def sub_keys(col, order):
    """One key column as integer arrays, the most significant first, every one 0 under a null: (validity,
    value) for a fixed-width integer column; (validity, bytes 0-7 big-endian zero-padded, bytes 8-15
    likewise, length) for a byte column of cells up to 16 bytes. With zero padding the last three order the
    cells as unsigned bytes with a proper prefix first."""
    n = col.nrows
    valid = valid_rows(col)
    if col.kind in FIXED:
        assert order in (SIGNED, UNSIGNED), order
        w = FIXED[col.kind]
        dt = {(1, SIGNED): np.int8, (4, SIGNED): np.int32, (8, SIGNED): np.int64,
              (1, UNSIGNED): np.uint8, (4, UNSIGNED): np.uint32, (8, UNSIGNED): np.uint64}[w, order]
        v = np.ascontiguousarray(col.values).view(np.uint8).reshape(-1)[:n * w].view(dt)
        return [valid.astype(np.uint8), np.where(valid, v, 0).astype(np.int64 if order == SIGNED else np.uint64)]
    assert col.kind in (BYTES32, BYTES64), col.kind
    off = np.asarray(col.offsets).astype(np.int64)
    lens = np.where(valid, off[1:] - off[:-1], 0)
    assert n == 0 or (0 <= lens.min() and lens.max() <= 16), "byte cells of at most 16 bytes"
    padded = np.zeros((n, 16), dtype=np.uint8)
    total = int(lens.sum())
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    data = np.asarray(col.values, dtype=np.uint8) if col.values is not None else np.zeros(0, dtype=np.uint8)
    padded[np.repeat(np.arange(n), lens), within] = data[np.repeat(off[:-1], lens) + within]
    words = padded.view(">u8").astype(np.uint64)
    return [valid.astype(np.uint8), words[:, 0], words[:, 1], lens.astype(np.uint64)]


def sort_indices_arrays(columns, orders=None):
    """`_sortrows.sort_indices` for fixed-width integer keys (SIGNED or UNSIGNED) and byte keys of cells up
    to 16 bytes, with optional validity: (perm uint32, tied). `np.lexsort` is stable and takes its last key
    first: nulls (validity 0) come first and rows equal on every key keep their input order."""
    orders = [SIGNED] * len(columns) if orders is None else list(orders)
    keys = [k for c, o in zip(columns, orders) for k in sub_keys(c, o)]      # the most significant first
    n = columns[0].nrows
    if n == 0:
        return np.zeros(0, dtype=np.uint32), 0
    perm = np.lexsort(tuple(reversed(keys)))
    # the rows that equal another row on every key: np.unique over the stacked keys, one key at a time -- the
    # codes of the keys so far and the next key make one word whose distinct values are the distinct rows
    code = np.zeros(n, dtype=np.uint64)
    for k in keys:
        if k.min() == k.max():
            continue                                                       # one value: tells no rows apart
        inverse = np.unique(k, return_inverse=True)[1].reshape(-1).astype(np.uint64)
        pair = code * np.uint64(int(inverse.max()) + 1) + inverse         # codes are below n: below 2^64
        code = np.unique(pair, return_inverse=True)[1].reshape(-1).astype(np.uint64)
    counts = np.unique(code, return_counts=True)[1]
    return perm.astype(np.uint32), int(counts[counts > 1].sum())


def keyed_diff_arrays(left, right, left_target=None, right_target=None, keep=False):
    """`_keyeddiff.keyed_diff` over integer keys that are unique on each side and integer targets (None: the
    null column), without validity: ((left rows, right rows, status), counts, dupes) -- the pairs as three
    arrays in the canonical order with -1 for an absent side, {status: joined rows} and (0, 0)."""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    nl, nr = left.size, right.size
    assert np.unique(left).size == nl and np.unique(right).size == nr, "keys are unique on each side"
    _, li, ri = np.intersect1d(left, right, assume_unique=True, return_indices=True)
    partner = np.full(nl, -1, dtype=np.int64)
    partner[li] = ri
    status = np.full(nl, REMOVED, dtype=np.uint8)                # rule 2: the right row is absent
    if left_target is None and right_target is None:
        differ = np.zeros(li.size, dtype=bool)                     # rule 3
    elif left_target is None or right_target is None:
        differ = np.ones(li.size, dtype=bool)                      # rule 4: None differs from every digest
    else:
        differ = np.asarray(left_target)[li] != np.asarray(right_target)[ri]
    status[li] = np.where(differ, MODIFIED, UNCHANGED)
    alone = np.ones(nr, dtype=bool)
    alone[ri] = False
    only = np.nonzero(alone)[0]                                    # rule 1: the left row is absent
    lrows = np.concatenate([np.arange(nl, dtype=np.int64), np.full(only.size, -1, dtype=np.int64)])
    rrows = np.concatenate([partner, only])
    status = np.concatenate([status, np.full(only.size, ADDED, dtype=np.uint8)])
    counts = {s: int((status == s).sum()) for s in (UNCHANGED, ADDED, REMOVED, MODIFIED)}
    if not keep:
        emitted = status != UNCHANGED
        lrows, rrows, status = lrows[emitted], rrows[emitted], status[emitted]
    return (lrows, rrows, status), counts, (0, 0)


def last_and_absent(mine, other):
    flags = np.zeros(mine.size, dtype=np.uint8)
    if mine.size:
        values, first_reversed = np.unique(mine[::-1], return_index=True)
        last = mine.size - 1 - first_reversed
        flags[last[~np.isin(values, other)]] = 1
    return flags


def row_diff_arrays(base, head):
    """`_rowhash.compute_new_row_indices` over integer keys as flags: (removed, added, (removed rows, added
    rows)) -- one uint8 per base / head row, 1 at the last occurrence of a key on its side that the other
    side lacks."""
    base, head = np.asarray(base, dtype=np.int64), np.asarray(head, dtype=np.int64)
    removed, added = last_and_absent(base, head), last_and_absent(head, base)
    return removed, added, (int(removed.sum()), int(added.sum()))


# ---------------------------------------------------------------- generators: columns
def text_column(lengths, seed, kind=BYTES32, alphabet=(0, 256), validity=None, validity_bit=0):
    """A byte column whose row r has lengths[r] random bytes of the alphabet [lo, hi), from offset 0."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    values = rng.integers(*alphabet, size=int(offsets[-1]), dtype=np.uint8)
    return Column(kind, lengths.size, values, offsets.astype(np.int32 if kind == BYTES32 else np.int64), validity, 0,
                  validity_bit)


def cells_column(cells, kind=BYTES32, validity=None, validity_bit=0):
    """A byte column from a list of bytes."""
    off = np.zeros(len(cells) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cells], out=off[1:])
    return Column(kind, len(cells), np.frombuffer(b"".join(cells), dtype=np.uint8), off.astype(np.int32 if kind == BYTES32 else np.int64),
                  validity, 0, validity_bit)


def with_nulls(c, seed, bit=5):
    """A third of the rows null, the validity bitmap's row 0 at `bit`."""
    rng = np.random.default_rng(seed)
    return c._replace(validity=packed_at(rng.random(c.nrows) > 1 / 3, bit, rng), validity_bit=bit)


# ---------------------------------------------------------------- generators: row hashes
def hash_frame(n, planted=(), seed=0):
    """An int32 column and a BYTES32 text column of 0-8 B cells: every row is 4-12 bytes but the planted
    (row, row bytes) ones."""
    rng = np.random.default_rng(7919 * seed + n)
    lengths = rng.integers(0, 9, size=n)
    for row, row_bytes in planted:
        lengths[row] = row_bytes - 4
    return [Column(4, n, rng.integers(-2**31, 2**31, size=n).astype(np.int32)), text_column(lengths, 7919 * seed + n + 1)]


# ---------------------------------------------------------------- generators: row diff
def row_diff_keys(nbase, nhead, tail, seed=0):
    """(base, head) integer keys. The keys are unique apart from 1 % repeats inside base; head holds the
    base rows before the last `tail` in another order, 1 % of them changed, then new rows: every one of the
    last `tail` head rows is new and every one of the last `tail` base rows is removed."""
    rng = np.random.default_rng(104729 * seed + 31 * nbase + nhead)
    pool = rng.permutation(4 * (nbase + nhead) + 8).astype(np.int64)
    base, fresh = pool[:nbase].copy(), pool[nbase:]
    shared = min(max(nbase - tail, 0), max(nhead - tail, 0))
    if shared > 7:
        dup = rng.integers(0, shared, size=shared // 100)
        base[dup] = base[(dup + 7) % shared]
    head = np.concatenate([base[:shared][rng.permutation(shared)], fresh[:nhead - shared]])
    changed = np.nonzero(rng.random(shared) < 0.01)[0]
    head[changed] = fresh[nhead - shared:nhead - shared + changed.size]
    return base, head


# ---------------------------------------------------------------- generators: keyed diff
def keyed_int_case(nl, nr, seed=0):
    """(left, right, left target, right target) integers. Unique keys; the right side is a permutation of
    the left with about a fifth of the rows dropped, as many added and a fifth of the targets changed."""
    rng = np.random.default_rng(15485863 * seed + 1000 * nl + nr)
    keys = rng.permutation(4 * (nl + nr) + 8)[:nl + nr].astype(np.int64)     # nl left keys, then fresh ones
    shared = min(nl, nr) - min(nl, nr) // 5
    right = rng.permutation(np.concatenate([rng.permutation(keys[:nl])[:shared], keys[nl:nl + nr - shared]]))
    left = keys[:nl]
    rt = right * 7 + 3
    rt[rng.random(nr) < 0.2] += 1
    return left, right, left * 7 + 3, rt


SPLIT_GROUPS = [(1, 2), (2, 3), (1, 65), (1, 300)]     # (left, right) multiplicity
PAST_GROUPS = SPLIT_GROUPS[:3]


def dupes_split_case(nl, nr, edge, seed=0):
    """(left, right, left target, right target, groups): integer keys that are unique but for planted groups
    of duplicates, and targets of three values. groups: a list of (kind, (left, right) multiplicity, key,
    the group's right rows ascending).

    "past": one copy of every group of PAST_GROUPS, its right rows a run of neighbours from right row
    edge + 1 on. "split": one copy of every group of SPLIT_GROUPS with right rows on both sides of right row
    `edge` -- the (1, 2) group at exactly edge - 1 and edge, the others about 3 / 5 before and 2 / 5 past it
    at random places. (The rows past `edge` have to hold the past runs and parts: 219 rows.)"""
    rng = np.random.default_rng(32452843 * seed + 1000 * nl + nr)
    need_past = sum(b for _, b in PAST_GROUPS) + 1 + sum(b - (3 * b) // 5 for _, b in SPLIT_GROUPS[1:])
    assert nr - edge - 1 >= need_past and edge - 1 >= sum((3 * b) // 5 for _, b in SPLIT_GROUPS[1:]), (nr, edge)
    assert nl >= 2 * sum(a for a, _ in SPLIT_GROUPS)
    right = np.full(nr, -1, dtype=np.int64)
    left = np.full(nl, -1, dtype=np.int64)
    groups, key, at = [], 10**12, edge + 1
    for mult in PAST_GROUPS:
        rows = np.arange(at, at + mult[1])
        at += mult[1]
        groups.append(("past", mult, key, rows))
        key += 1
    free_past = rng.permutation(np.arange(at, nr))
    free_before = rng.permutation(edge - 1)
    for mult in SPLIT_GROUPS:
        if mult == (1, 2):
            rows = np.array([edge - 1, edge])
        else:
            before = (3 * mult[1]) // 5
            rows = np.sort(np.concatenate([free_before[:before], free_past[:mult[1] - before]]))
            free_before, free_past = free_before[before:], free_past[mult[1] - before:]
        groups.append(("split", mult, key, rows))
        key += 1
    left_free = rng.permutation(nl)
    for _, (a, _), k, rows in groups:
        right[rows] = k
        left[left_free[:a]] = k
        left_free = left_free[a:]
    # the other rows: unique keys, four fifths of the left ones matched where the right side has room
    rest_l, rest_r = np.nonzero(left < 0)[0], np.nonzero(right < 0)[0]
    keys = rng.permutation(4 * (nl + nr) + 8)[:rest_l.size + rest_r.size].astype(np.int64)
    matched = min((4 * rest_l.size) // 5, rest_r.size)
    left[rest_l] = keys[:rest_l.size]
    right[rng.permutation(rest_r)] = np.concatenate([rng.permutation(keys[:rest_l.size])[:matched],
                                                     keys[rest_l.size:rest_l.size + rest_r.size - matched]])
    return left, right, rng.integers(0, 3, size=nl), rng.integers(0, 3, size=nr), groups


# ---------------------------------------------------------------- generators: take
BIG_CELL_ROW, BIG_CELL = 7, 5000


def take_case(nout, big_at=(), nrows=70001, seed=0):
    """(columns, idx0, idx1, plan): a left frame of `nrows` rows -- an int64 column with nulls, a BYTES32
    column of 0-7 B cells, a boolean column -- and a right frame of nrows - 3 rows of the same kinds, every
    output column the left one through idx0 with the right one through idx1 as its fallback. An eighth of
    the indices of each array are absent. big_at: output rows that select the left text column's one
    5 000 B cell (source row 7, present)."""
    rng = np.random.default_rng(49979687 * seed + 1000 * nrows + nout % 1000)

    def side(n, big):
        lengths = rng.integers(0, 8, size=n)
        valid = rng.random(n) > 0.2
        if big:
            lengths[BIG_CELL_ROW], valid[BIG_CELL_ROW] = BIG_CELL, True
        return [Column(8, n, rng.integers(-2**63, 2**63, size=n).astype(np.int64), None, np.packbits(rng.random(n) > 0.2, bitorder="little")),
                text_column(lengths, int(rng.integers(1 << 30)), alphabet=(97, 123), validity=np.packbits(valid, bitorder="little")),
                Column(BOOL, n, np.packbits(rng.random(n) < 0.5, bitorder="little"), None, np.packbits(rng.random(n) > 0.2, bitorder="little"))]

    nright = max(1, nrows - 3)
    cols = side(nrows, bool(len(big_at))) + side(nright, False)
    idx0 = rng.integers(0, nrows, size=nout).astype(np.uint32)
    idx1 = rng.integers(0, nright, size=nout).astype(np.uint32)
    idx0[rng.random(nout) < 1 / 8] = NONE
    idx1[rng.random(nout) < 1 / 8] = NONE
    for row in big_at:
        idx0[row] = BIG_CELL_ROW
    return cols, idx0, idx1, [(c, 0, 3 + c, 1) for c in range(3)]


# ---------------------------------------------------------------- generators: sort
EQUAL_KEY = 0x4142434445464748


def int64_keys(n, seed=0):
    """Random int64 keys over the whole range, the extremes, 0 and -1 among the first rows."""
    rng = np.random.default_rng(67867967 * seed + n)
    keys = rng.integers(-2**63, 2**63, size=n).astype(np.int64)
    edges = np.array([-2**63, 2**63 - 1, 0, -1], dtype=np.int64)
    keys[:min(n, 4)] = edges[:min(n, 4)]
    return keys


def grouped_keys(n, distinct, seed=0):
    """(an int32 column of at most `distinct` values on both sides of 0 with a third of the rows null at
    validity_bit 5, an int64 column of random keys)."""
    rng = np.random.default_rng(86028121 * seed + n)
    first = ((rng.integers(0, distinct, size=n) - distinct // 2) * 21001).astype(np.int32)
    return with_nulls(Column(4, n, first), 86028121 * seed + n + 1), Column(8, n, int64_keys(n, seed + 1))


def one_low_row(n, byte):
    """Every key EQUAL_KEY but the last row's, whose byte `byte` is one lower: it sorts first."""
    keys = np.full(n, EQUAL_KEY, dtype=np.int64)
    if n:
        keys[-1] -= 1 << (8 * byte)
    return keys


def one_null_row(n):
    """The same key in every row, all valid but the last."""
    valid = np.ones(n, dtype=bool)
    valid[-1:] = False
    return Column(8, n, np.full(n, EQUAL_KEY, dtype=np.int64), None, np.packbits(valid, bitorder="little"))


def one_short_row(n):
    """b"abc" in every row but the last, which holds b"ab"."""
    lengths = np.full(n, 3, dtype=np.int64)
    lengths[-1:] = 2
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    values = np.tile(np.frombuffer(b"abc", dtype=np.uint8), n)[:int(offsets[-1])]
    return Column(BYTES32, n, values, offsets.astype(np.int32))


LADDER = [b"", b"a", b"a\0", b"a\0\0", b"a" + b"\0" * 6, b"a" + b"\0" * 7, b"a" + b"\0" * 8, b"a" + b"\0" * 14, b"a" + b"\0" * 15,
          b"b", b"ab", b"\xff", b"\x80", b"\x7f", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\0", b"abcdefghijklmno",
          b"abcdefghijklmnop", b"abcdefghijklmno\0", b"abcdefgi"]


def short_cells(n, seed=0):
    """Cells of 0, 7, 8, 9, 15 and 16 bytes over {0, 'a', 'b'} and the ladder of cells that differ only by
    trailing zero bytes, each drawn many times."""
    rng = np.random.default_rng(98764321 * seed + n)
    pool = list(LADDER)
    for length in (0, 7, 8, 9, 15, 16):
        pool += [bytes(rng.choice([0, 97, 98], size=length).astype(np.uint8)) for _ in range(6)]
    return [pool[i] for i in rng.integers(0, len(pool), size=n)]
