"""The CPU restatement the embedding tests compare with (tests/test_embedding.py, test_embedding_cpu.py): the
semantics of include/oxen_hash.h ("embedding similarity") in plain numpy, row by row. A column is an
`oxen_amd.tabular.Embedding` description over numpy arrays. Nothing here calls the library, and pyarrow is not
needed.

A row is None for a null, "wrong" for a valid list row whose length is not dim (never read), else its dim
float32 values. The similarity of a row is float32 throughout: dot, nx and nq summed in float32 in index order,
sim = dot / sqrt(nx * nq), clamped to [-1, 1] by comparisons that let a NaN through. The order key is the bitwise
NOT of the row sort's float32 word; the order is the stable ascending sort of the keys.
"""
import numpy as np

FIXED, LIST32, LIST64 = 0, 1, 2
NULL_KEY = 0xFFFFFFFF
TAKE_NULL = 0xFFFFFFFF
WRONG = "wrong"


def bits(packed, bit0, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n].astype(bool)


def packed_at(mask, bit0=0, fill=1):
    """The Arrow bitmap of `mask` with row 0 at bit `bit0`; the bits around the rows are `fill`."""
    mask = np.asarray(mask, dtype=bool)
    total = 8 * -(-(bit0 + mask.size) // 8)
    all_bits = np.full(total, bool(fill))
    all_bits[bit0:bit0 + mask.size] = mask
    return np.packbits(all_bits, bitorder="little")


def rows(emb):
    """One entry per row: None, WRONG, or the row's float32 values."""
    n, d = int(emb.nrows), int(emb.dim)
    valid = np.ones(n, dtype=bool) if emb.validity is None else bits(emb.validity, emb.validity_bit, n)
    values = np.asarray(emb.values, dtype=np.float32).reshape(-1) if emb.values is not None else np.zeros(0, np.float32)
    out = []
    for r in range(n):
        if not valid[r]:
            out.append(None)
        elif emb.layout == FIXED:
            out.append(values[r * d:(r + 1) * d])
        else:
            s, e = int(emb.offsets[r]), int(emb.offsets[r + 1])
            out.append(values[s:e] if e - s == d else WRONG)
    return out


def stats_of(picked, nrows):
    """stats4 over the rows a call names: used, null, wrong, the smallest wrong row (nrows when none)."""
    wrong = [r for r, v in picked if isinstance(v, str)]
    return (sum(1 for _, v in picked if v is not None and not isinstance(v, str)), sum(1 for _, v in picked if v is None),
            len(wrong), min(wrong) if wrong else nrows)


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def float_word(b):
    """sort_keys.hpp's encode_float32: every NaN one NaN above +inf, -0.0 as +0.0, then the total-order flip."""
    if (b & 0x7FFFFFFF) > 0x7F800000:
        b = 0x7FC00000
    if b == 0x80000000:
        b = 0
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def order_key(sim):
    """The key of a valid row's similarity (a float32, or its bits as an int)."""
    b = sim if isinstance(sim, int) else f32_bits(sim)
    return ~float_word(b) & 0xFFFFFFFF


def stable_order(keys):
    return np.argsort(np.asarray(keys, dtype=np.uint32), kind="stable").astype(np.uint32)


def cosine(x, q):
    """One row, float32 throughout, summed in index order."""
    dot = nx = nq = np.float32(0)
    with np.errstate(all="ignore"):
        for a, b in zip(np.asarray(x, np.float32), np.asarray(q, np.float32)):
            dot = np.float32(dot + a * b)
            nx = np.float32(nx + a * a)
            nq = np.float32(nq + b * b)
        s = np.float32(dot / np.sqrt(np.float32(nx * nq)))
    if s > 1:
        s = np.float32(1)
    if s < -1:
        s = np.float32(-1)
    return s


class Ranked:
    def __init__(self, sim, validity, key, perm, stats):
        self.sim, self.validity, self.key, self.perm, self.stats = sim, validity, key, perm, stats


def finish(sim, valid, state_rows, nrows):
    """sim (0.0 where not valid), the validity bytes, the keys, the stable order and the stats."""
    sim = np.where(valid, sim, np.float32(0)).astype(np.float32)
    key = np.array([order_key(int(b)) if ok else NULL_KEY for b, ok in zip(sim.view(np.uint32).tolist(), valid.tolist())], dtype=np.uint32)
    return Ranked(sim, np.packbits(valid, bitorder="little"), key, stable_order(key), stats_of(state_rows, nrows))


def similarity(emb, query):
    """Row by row."""
    rs = rows(emb)
    valid = np.array([v is not None and not isinstance(v, str) for v in rs], dtype=bool)
    sim = np.array([cosine(v, query) if ok else 0 for v, ok in zip(rs, valid)], dtype=np.float32)
    return finish(sim, valid, list(enumerate(rs)), int(emb.nrows))


def similarity_exact(emb, query):
    """The same for integer-valued inputs whose sums are exact in any order (|values| <= 8, dim <= 4097): the sums
    in float64, then the float32 divide and square root -- vectorised, for frames of many rows. Fixed layout."""
    assert emb.layout == FIXED
    n, d = int(emb.nrows), int(emb.dim)
    x = np.asarray(emb.values, dtype=np.float32).reshape(-1)[:n * d].reshape(n, d).astype(np.float64)
    q = np.asarray(query, dtype=np.float64)
    dot, nx, nq = (x @ q).astype(np.float32), (x * x).sum(axis=1).astype(np.float32), np.float32((q * q).sum())
    with np.errstate(all="ignore"):
        sim = (dot / np.sqrt(nx * nq)).astype(np.float32)
    sim = np.where(sim > 1, np.float32(1), np.where(sim < -1, np.float32(-1), sim)).astype(np.float32)
    valid = np.ones(n, dtype=bool) if emb.validity is None else bits(emb.validity, emb.validity_bit, n)
    state = [(r, 0.0 if ok else None) for r, ok in enumerate(valid.tolist())]
    sim = np.where(valid, sim, np.float32(0)).astype(np.float32)
    u = sim.view(np.uint32).astype(np.uint64)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC00000, u)
    u = np.where(u == 0x80000000, 0, u)
    word = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    key = np.where(valid, ~word & 0xFFFFFFFF, NULL_KEY).astype(np.uint32)
    return Ranked(sim, np.packbits(valid, bitorder="little"), key, stable_order(key), stats_of(state, n))


def mean(emb, idx):
    """(mean or None when no row is used, stats): float32 sums in idx order, one float32 division."""
    rs = rows(emb)
    picked = [(int(r), rs[int(r)]) for r in idx]
    used = [v for _, v in picked if v is not None and not isinstance(v, str)]
    if not used:
        return None, stats_of(picked, int(emb.nrows))
    total = np.zeros(int(emb.dim), dtype=np.float32)
    for v in used:
        total = (total + v).astype(np.float32)
    return (total / np.float32(len(used))).astype(np.float32), stats_of(picked, int(emb.nrows))


def take(emb, idx):
    """(values nout * dim float32, validity bytes, stats): an absent index, a null row and a row that is not read
    give zeros and validity bit 0."""
    rs = rows(emb)
    d = int(emb.dim)
    out = np.zeros((len(idx), d), dtype=np.float32)
    valid = np.zeros(len(idx), dtype=bool)
    picked = []
    for o, r in enumerate(np.asarray(idx, dtype=np.uint32).tolist()):
        v = None if r == TAKE_NULL else rs[r]
        picked.append((r, v))
        if v is not None and not isinstance(v, str):
            out[o], valid[o] = v, True
    return out.reshape(-1), np.packbits(valid, bitorder="little"), stats_of(picked, int(emb.nrows))


def page_rows(nrows, page_size, page_num):
    first = min((max(page_num, 1) - 1) * page_size, nrows)
    return first, min(page_size, nrows - first)
