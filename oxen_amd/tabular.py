"""Row hashes of a data frame from its columns, the row set-diff and the keyed diff (`oxen diff` / `oxen df`).

The reference (core/df/tabular.rs:816-945 `df_hash_rows`, `df_hash_rows_on_cols`) walks a frame row by
row: `any_val_to_bytes` (:651-675) of every cell appended to one buffer, `hasher::hash_buffer` of it, the
hex string stored; repositories/diffs.rs:1023-1074 `compute_new_row_indices` then builds two
HashMap<String, u32> over those strings. Here a frame stays columnar and `oxh_row_hashes_*` hashes every
row on the device straight from the columns; `oxh_row_diff_*` answers the set question on the device too.

`oxh_keyed_diff_*` is `oxen diff --keys ... --targets ...` after the hashing (diffs.rs:881-901 `diff_dfs`,
repositories/diffs/join_diff.rs): the full join of the two frames on their key hashes, every joined row
labelled added / removed / modified / unchanged, and the summary counts -- `keyed_diff_digests`, `diff_dfs`.

`oxh_take_columns_*` builds what that diff returns, `TabularDiff.contents`: a take of both frames' columns by
the joined rows' indices, null indices and a fallback source (the keys' coalesce) included -- `take`,
`take_device`, `diff_contents`, `diff_dfs_contents`, and `columns_to_arrow` back to pyarrow.

`oxh_sort_rows_*` is the reference's `sort_df_on_keys` of that frame (join_diff.rs:146-163) and `oxen df --sort`:
a stable multi-column sort of the rows on the device that returns a permutation -- `sort_indices`,
`sort_indices_device`, `sort_by`, and `sort=True` of `diff_contents` / `diff_dfs_contents`.

`oxh_group_rows_*` groups the rows of a frame by equality on key columns, which is what `oxen df --unique`,
`--unique_count` (core/df/tabular.rs:424-433) and `n_duped_rows` (:263-271) read off -- `group_rows`,
`group_rows_device`, `unique`, `unique_count`, `is_duplicated`, `n_duped_rows`.

`oxh_filter_rows_*` is `oxen df --filter` (core/df/tabular.rs:404-422 `filter_df`, the parser of
core/df/filter.rs): the rows for which terms `column OP literal`, joined by && / || and folded left to right,
give true, as ascending row indices for the take and / or an Arrow bitmap -- `parse_filter`, `filter_terms`,
`filter_rows`, `filter_rows_device`, `filter_df`.

`oxh_embedding_*` is the embedding query (repositories/workspaces/data_frames/embeddings.rs `query`,
`nearest_neighbors`, `get_avg_embedding`): the mean of the vectors the filter selects, the cosine similarity of
every row with it, the rows ranked from the most similar on and one page of them with its own vectors --
`Embedding`, `embedding`, `embedding_from_arrow`, `embedding_mean`, `cosine_similarity`, `embedding_take`,
`nearest_neighbors`, `sort_by_similarity`, each with a `_device` twin.

`oxh_concat_columns_*` is the first and the last step of `oxen df`'s chain (core/df/tabular.rs:443-589): `--vstack`
(polars' vertical concat) and `--slice` / `--head` / `--tail` / the page of a data-frame view are row ranges of one
or more frames written one after the other, as copies -- `concat`, `concat_device`, `slice_range`, `parse_slice`,
`slice_rows`, `head`, `tail`, `page`, `vstack`, each frame function with a `_device` twin.

`oxh_csv_*` reads a CSV file into such columns on the device (`read_csv`, `read_csv_device`, `CsvFile`) and
`oxh_write_csv_*` writes them back as the file's bytes, which is how every path of the reference ends (`write_df`,
core/df/tabular.rs:1492-1547) -- `write_csv`, `write_csv_device`, `write_df`; `oxh_write_json_*` as JSON Lines or one
JSON array (`write_df`'s jsonl / ndjson / json arms, and the text of a data-frame view) -- `write_jsonl`, `write_json` and
their `_device` forms.

A frame is an ordered mapping from column name to `Column`. A row's bytes are, over the columns in the
frame's order: nothing for a null, the raw little-endian bytes of Int8 / Int32 / Float32 / Int64 /
Float64 / Datetime(ms), one byte 0 or 1 for a boolean, the UTF-8 bytes of a string. Every other dtype
goes through `to_string()` in the reference: render such a column to strings yourself and pass it as a
byte column (polars' Display is not restated here). Cells are not delimited, as in the reference.
"""
from __future__ import annotations

import ctypes
import re
from typing import Any, Mapping, NamedTuple, Optional, Sequence

import numpy as np

from . import _capi
from ._capi import (OXH_COL_BOOL, OXH_COL_BYTES32, OXH_COL_BYTES64, OXH_COL_FIXED1, OXH_COL_FIXED4,  # noqa: F401
                    OXH_COL_FIXED8, OXH_SORT_FLOAT, OXH_SORT_SIGNED, OXH_SORT_UNSIGNED)

_BYTES = (OXH_COL_BYTES32, OXH_COL_BYTES64)
_WIDTH = {OXH_COL_FIXED1: 1, OXH_COL_FIXED4: 4, OXH_COL_FIXED8: 8}


class Column(NamedTuple):
    """One column as `oxh_row_hashes_*` takes it (numpy arrays for the host form, torch tensors on the
    device for the device form). values: the nrows cells of a fixed-width column (any dtype of that
    width), the bit-packed booleans (uint8, LSB first), or the bytes of a byte column (uint8);
    offsets: nrows + 1 int32 / int64 for a byte column; validity: an Arrow validity bitmap (uint8) or
    None for no nulls; value_bit / validity_bit: the bit of row 0 in a boolean's values / in validity."""
    kind: int
    nrows: int
    values: Any
    offsets: Any = None
    validity: Any = None
    value_bit: int = 0
    validity_bit: int = 0


def _pack(mask) -> np.ndarray:
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def column(values, validity=None) -> Column:
    """A Column from host data: a numpy array of int8 / int32 / float32 / int64 / float64 /
    datetime64[ms] / bool, or a sequence of str / bytes / None (a string column; None is a null).
    validity: a boolean mask (True = present) or None."""
    mask = None if validity is None else _pack(validity)
    if not isinstance(values, np.ndarray):
        items = list(values)
        present = [v is not None for v in items]
        raw = [b"" if v is None else (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for v in items]
        offsets = np.zeros(len(raw) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in raw], out=offsets[1:])
        wide = int(offsets[-1]) > np.iinfo(np.int32).max
        data = np.frombuffer(b"".join(raw), dtype=np.uint8)
        if mask is None and not all(present):
            mask = _pack(present)
        return Column(OXH_COL_BYTES64 if wide else OXH_COL_BYTES32, len(raw), data,
                      offsets if wide else offsets.astype(np.int32), mask)
    a = np.ascontiguousarray(values)
    if a.ndim != 1:
        raise _capi.OxenError("a column is one-dimensional", _capi.OXH_ERR_INVALID)
    if a.dtype == np.bool_:
        return Column(OXH_COL_BOOL, a.size, _pack(a), None, mask)
    if a.dtype in (np.dtype(np.int8), np.dtype(np.int32), np.dtype(np.float32), np.dtype(np.int64), np.dtype(np.float64),
                   np.dtype("datetime64[ms]")):
        return Column(a.dtype.itemsize, a.size, a, None, mask)
    raise _capi.OxenError(f"dtype {a.dtype} has no raw row bytes in the reference (it goes through to_string()): "
                          "cast the column to strings", _capi.OXH_ERR_INVALID)


def _as_columns(columns) -> list:
    cols = [c if isinstance(c, Column) else column(c) for c in columns]
    if cols and any(c.nrows != cols[0].nrows for c in cols):
        raise _capi.OxenError("the columns of a frame have one row count", _capi.OXH_ERR_INVALID)
    return cols


def _tables(cols, ptr):
    """The five parallel arrays of the ABI; ptr(x) = the address of an array / tensor, None for None."""
    n = len(cols)
    kinds = (ctypes.c_uint32 * max(n, 1))(*[int(c.kind) for c in cols])
    values = (ctypes.c_void_p * max(n, 1))(*[ptr(c.values) for c in cols])
    offsets = (ctypes.c_void_p * max(n, 1))(*[ptr(c.offsets) if c.kind in _BYTES else None for c in cols])
    validity = (ctypes.c_void_p * max(n, 1))(*[ptr(c.validity) for c in cols])
    bits = (ctypes.c_uint64 * max(2 * n, 1))()
    for k, c in enumerate(cols):
        bits[2 * k], bits[2 * k + 1] = int(c.value_bit), int(c.validity_bit)
    return kinds, values, offsets, validity, bits


def _handle(ctx):
    # without a device there is no context to make: the library answers OXH_ERR_NODEVICE (after its
    # argument checks, which need neither)
    import torch

    from .hasher import default_context

    if ctx is not None:
        return ctx.handle
    return default_context().handle if torch.cuda.is_available() else None


def row_hashes(columns: Sequence, ctx: Optional[_capi.Context] = None) -> np.ndarray:
    """oxh_row_hashes_host: (n, 2) uint64 rows of (lo, hi), the XXH3-128 of every row's bytes.
    columns: `Column`s (or what `column` takes) in the frame's order, in host memory."""
    cols = _as_columns(columns)
    nrows = cols[0].nrows if cols else 0
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    out = np.zeros((nrows, 2), dtype=np.uint64)
    _capi.check(_capi.lib().oxh_row_hashes_host(_handle(ctx), nrows, len(cols), *_tables(cols, ptr),
                                                out.ctypes.data_as(_capi._u64p)), "oxh_row_hashes_host")
    return out


def row_hashes_device(columns: Sequence[Column], stream=None, ctx: Optional[_capi.Context] = None):
    """oxh_row_hashes_device: the same over `Column`s whose values / offsets / validity are torch tensors
    on the device; returns an (n, 2) int64 device tensor holding the raw u64 words. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    cols = list(columns)
    nrows = cols[0].nrows if cols else 0
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    out = torch.empty((nrows, 2), dtype=torch.int64, device=device)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    _capi.check(_capi.lib().oxh_row_hashes_device(_handle(ctx), nrows, len(cols), *_tables(cols, ptr),
                                                  out.data_ptr() if nrows else None, _stream(stream)),
                "oxh_row_hashes_device")
    return out


def row_hash_strings(digests) -> list:
    """The reference's row-hash strings: `format!("{:x}")` of the u128, lowercase and unpadded
    (oxh_format_hex)."""
    a = np.ascontiguousarray(digests, dtype=np.uint64).reshape(-1, 2)
    buf = ctypes.create_string_buffer(33)
    L = _capi.lib()
    out = []
    for lo, hi in a.tolist():
        n = L.oxh_format_hex(lo, hi, buf)
        out.append(buf.raw[:n].decode())
    return out


def df_hash_rows(frame: Mapping, ctx: Optional[_capi.Context] = None) -> np.ndarray:
    """tabular.rs:816-878: the hash of every row over all the frame's columns, in its schema order."""
    return row_hashes(list(frame.values()), ctx=ctx)


def df_hash_rows_on_cols(frame: Mapping, hash_fields, ctx: Optional[_capi.Context] = None) -> Optional[np.ndarray]:
    """tabular.rs:880-945: the hash of every row over the columns named in hash_fields. The frame's
    column order is kept, not that of hash_fields; names that are not in the frame are ignored; None
    (the reference's null column) when no named column is present."""
    wanted = set(hash_fields)
    cols = [c for name, c in frame.items() if name in wanted]
    if not cols:
        return None
    return row_hashes(cols, ctx=ctx)


def _digests(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 2:
        if a.size == 0:
            return a.reshape(0, 2)
        raise _capi.OxenError("digests must be an (n, 2) uint64 array of (lo, hi) rows", _capi.OXH_ERR_INVALID)
    return a


def row_diff(base_digests, head_digests, ctx: Optional[_capi.Context] = None):
    """oxh_row_diff_host over two (n, 2) digest tables: (added, removed), ascending uint32 row indices --
    the last row of every distinct head digest that base lacks, and the mirror image."""
    base, head = _digests(base_digests), _digests(head_digests)
    removed = np.zeros(base.shape[0], dtype=np.uint32)
    added = np.zeros(head.shape[0], dtype=np.uint32)
    counts = np.zeros(2, dtype=np.uint64)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _capi.check(_capi.lib().oxh_row_diff_host(_handle(ctx), base.ctypes.data_as(_capi._u64p) if base.size else None,
                                              base.shape[0], head.ctypes.data_as(_capi._u64p) if head.size else None,
                                              head.shape[0], removed.ctypes.data_as(u32p) if base.size else None,
                                              added.ctypes.data_as(u32p) if head.size else None,
                                              counts.ctypes.data_as(_capi._u64p)), "oxh_row_diff_host")
    return added[:int(counts[1])], removed[:int(counts[0])]


def row_diff_device(d_base, d_head, stream=None, ctx: Optional[_capi.Context] = None):
    """oxh_row_diff_device over two (n, 2) 64-bit device tensors: (added, removed, counts) -- one uint8
    flag per head / base row on the device (1 = reported) and counts = (added rows, removed rows)."""
    import torch

    from .device import _require_cuda, _stream

    _require_cuda(d_base, d_head)
    for t in (d_base, d_head):
        if t.element_size() != 8 or t.numel() % 2 or not t.is_contiguous():
            raise _capi.OxenError("digest tables must be contiguous 64-bit (n, 2) tensors", _capi.OXH_ERR_INVALID)
    nbase, nhead = d_base.numel() // 2, d_head.numel() // 2
    removed = torch.zeros(nbase, dtype=torch.uint8, device=d_base.device)
    added = torch.zeros(nhead, dtype=torch.uint8, device=d_head.device)
    counts = np.zeros(2, dtype=np.uint64)
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    _capi.check(_capi.lib().oxh_row_diff_device(_handle(ctx), ptr(d_base), nbase, ptr(d_head), nhead, ptr(removed), ptr(added),
                                                counts.ctypes.data_as(_capi._u64p), _stream(stream)), "oxh_row_diff_device")
    return added, removed, (int(counts[1]), int(counts[0]))


def compute_new_row_indices(base: Mapping, head: Mapping, ctx: Optional[_capi.Context] = None):
    """diffs.rs:1023-1074 over two frames: (added, removed), each ascending -- two row-hash calls and one
    diff call."""
    return row_diff(df_hash_rows(base, ctx=ctx), df_hash_rows(head, ctx=ctx), ctx=ctx)


# ---------------------------------------------------------------- keyed diff
STATUS_NAMES = ("unchanged", "added", "removed", "modified")   # by OXH_DIFF_* code


class KeyedDiff(NamedTuple):
    """The classified joined rows of a keyed diff, in the canonical order (the left rows ascending, each
    followed by its pairs or its one (l, none); then the right-only rows ascending), and its summary.
    left_rows / right_rows: -1 = absent; status: an index into STATUS_NAMES. added / removed / modified /
    unchanged count all joined rows, emitted or not; dupes_left / dupes_right are the rows whose key
    occurs more than once on their own side."""
    left_rows: Any
    right_rows: Any
    status: Any
    added: int
    removed: int
    modified: int
    unchanged: int
    dupes_left: int
    dupes_right: int


def _key0_valid(v, nrows):
    """(bitmap, bit of row 0) from None, a boolean mask (True = present) or (Arrow bitmap, bit offset)."""
    if v is None:
        return None, 0
    if isinstance(v, tuple):
        bitmap, bit = v
        if bitmap is None:
            return None, 0
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        if bitmap.size * 8 < int(bit) + nrows:
            raise _capi.OxenError("a validity bitmap is shorter than its rows", _capi.OXH_ERR_INVALID)
        return bitmap, int(bit)
    mask = np.asarray(v, dtype=bool)
    if mask.shape != (nrows,):
        raise _capi.OxenError("a validity mask has one entry per row", _capi.OXH_ERR_INVALID)
    return _pack(mask), 0


def keyed_diff_digests(left_keys, right_keys, left_targets=None, right_targets=None, left_key0_valid=None,
                       right_key0_valid=None, keep_unchanged: bool = False, ctx: Optional[_capi.Context] = None) -> KeyedDiff:
    """oxh_keyed_diff_host over (n, 2) uint64 digest tables: the full join of the two sides on their key
    digests, every joined row labelled as join_diff.rs:458-484 (`test_function`) labels it, the unchanged
    ones left out unless keep_unchanged. Targets: None = the null column (no named target in that frame).
    *_key0_valid: the validity of the cell of keys[0] -- None (no nulls), a boolean mask, or (Arrow
    bitmap, bit of row 0). A row whose keys[0] is null on the left is `added`, else one whose keys[0] is
    null on the right `removed`, whatever it is paired with (the reference's behaviour).
    The first call has room for nleft + nright pairs, enough unless a key repeats on the right of a
    matched group; then the call is made again with the exact count."""
    lk, rk = _digests(left_keys), _digests(right_keys)
    nl, nr = lk.shape[0], rk.shape[0]
    lt = None if left_targets is None else _digests(left_targets)
    rt = None if right_targets is None else _digests(right_targets)
    if (lt is not None and lt.shape[0] != nl) or (rt is not None and rt.shape[0] != nr):
        raise _capi.OxenError("a target table has one row per key row", _capi.OXH_ERR_INVALID)
    lv, lbit = _key0_valid(left_key0_valid, nl)
    rv, rbit = _key0_valid(right_key0_valid, nr)
    bits = np.array([lbit, rbit], dtype=np.uint64)
    counts = np.zeros(8, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    flags = _capi.OXH_KEYED_DIFF_KEEP_UNCHANGED if keep_unchanged else 0
    capacity = nl + nr
    while True:
        left = np.empty(capacity, dtype=np.uint32)
        right = np.empty(capacity, dtype=np.uint32)
        status = np.empty(capacity, dtype=np.uint8)
        _capi.check(_capi.lib().oxh_keyed_diff_host(_handle(ctx), ptr(lk), nl, ptr(rk), nr, ptr(lt), ptr(rt), ptr(lv), ptr(rv),
                                                    bits.ctypes.data_as(_capi._u64p), flags, capacity, ptr(left), ptr(right),
                                                    ptr(status), counts.ctypes.data_as(_capi._u64p)), "oxh_keyed_diff_host")
        if int(counts[7]) == int(counts[0]):
            break
        capacity = int(counts[0])   # a key repeats on the right: now the exact count
    n = int(counts[7])
    none = _capi.OXH_KEYED_DIFF_NONE
    rows = lambda a: np.where(a[:n] == none, -1, a[:n].astype(np.int64))  # noqa: E731
    return KeyedDiff(rows(left), rows(right), status[:n].copy(), *(int(c) for c in counts[1:7]))


def keyed_diff_digests_device(d_left_keys, d_right_keys, d_left_targets=None, d_right_targets=None, d_left_key0_valid=None,
                              d_right_key0_valid=None, keep_unchanged: bool = False, stream=None,
                              ctx: Optional[_capi.Context] = None) -> KeyedDiff:
    """oxh_keyed_diff_device over (n, 2) 64-bit device tensors (targets: None = the null column;
    *_key0_valid: None or (uint8 device tensor holding an Arrow bitmap, bit of row 0)). The three arrays
    of the result are device tensors: left_rows / right_rows int32 holding the call's u32 words, so an
    absent side reads -1 (and a row index of 2^31 or more negative: view them as unsigned then), status
    uint8. Within one left row's pairs the right rows come in any order. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    valid = [v if v is not None else (None, 0) for v in (d_left_key0_valid, d_right_key0_valid)]
    tables = [d_left_keys, d_right_keys, d_left_targets, d_right_targets]
    tensors = [t for t in tables + [valid[0][0], valid[1][0]] if t is not None]
    _require_cuda(*tensors)
    for t in tables:
        if t is not None and (t.element_size() != 8 or t.numel() % 2 or not t.is_contiguous()):
            raise _capi.OxenError("digest tables must be contiguous 64-bit (n, 2) tensors", _capi.OXH_ERR_INVALID)
    nl, nr = d_left_keys.numel() // 2, d_right_keys.numel() // 2
    for t, n in ((d_left_targets, nl), (d_right_targets, nr)):
        if t is not None and t.numel() != 2 * n:
            raise _capi.OxenError("a target table has one row per key row", _capi.OXH_ERR_INVALID)
    for (bitmap, bit), n in zip(valid, (nl, nr)):
        if bitmap is not None and (bitmap.element_size() != 1 or not bitmap.is_contiguous() or bitmap.numel() * 8 < int(bit) + n):
            raise _capi.OxenError("a validity bitmap is a contiguous uint8 tensor that holds its rows' bits",
                                  _capi.OXH_ERR_INVALID)
    bits = np.array([int(valid[0][1]), int(valid[1][1])], dtype=np.uint64)
    counts = np.zeros(8, dtype=np.uint64)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    flags = _capi.OXH_KEYED_DIFF_KEEP_UNCHANGED if keep_unchanged else 0
    device = d_left_keys.device
    capacity = nl + nr
    while True:
        left = torch.empty(capacity, dtype=torch.int32, device=device)
        right = torch.empty(capacity, dtype=torch.int32, device=device)
        status = torch.empty(capacity, dtype=torch.uint8, device=device)
        _capi.check(_capi.lib().oxh_keyed_diff_device(_handle(ctx), ptr(d_left_keys), nl, ptr(d_right_keys), nr, ptr(d_left_targets),
                                                      ptr(d_right_targets), ptr(valid[0][0]), ptr(valid[1][0]),
                                                      bits.ctypes.data_as(_capi._u64p), flags, capacity, ptr(left), ptr(right),
                                                      ptr(status), counts.ctypes.data_as(_capi._u64p), _stream(stream)),
                    "oxh_keyed_diff_device")
        if int(counts[7]) == int(counts[0]):
            break
        capacity = int(counts[0])
    n = int(counts[7])
    return KeyedDiff(left[:n], right[:n], status[:n], *(int(c) for c in counts[1:7]))


def _as_frame(frame: Mapping) -> dict:
    return {name: c if isinstance(c, Column) else column(c) for name, c in frame.items()}


def _schema_diff(left: Mapping, right: Mapping):
    """diffs.rs:903-936 by column name: (added, removed, unchanged), each in its frame's order (the
    reference keeps them in HashSets)."""
    return [c for c in right if c not in left], [c for c in left if c not in right], [c for c in left if c in right]


def _keys_targets_smart_defaults(left: Mapping, right: Mapping, keys, targets):
    """diffs.rs:938-973."""
    keys, targets = list(keys), list(targets)
    added_cols, removed_cols, unchanged_cols = _schema_diff(left, right)
    if keys and not targets:
        targets = [c for c in unchanged_cols if c not in keys]
    elif targets and not keys:
        raise _capi.OxenError("Must specify at least one key column if specifying target columns.", _capi.OXH_ERR_INVALID)
    elif not keys:
        keys, targets = list(unchanged_cols), added_cols + removed_cols
    return keys, targets


def diff_dfs(left: Mapping, right: Mapping, keys: Sequence[str] = (), targets: Sequence[str] = (),
             ctx: Optional[_capi.Context] = None) -> KeyedDiff:
    """diffs.rs:881-901 `diff_dfs` up to the classified joined rows: the schema diff by column name, the
    smart defaults of :938-973 (keys only: targets = the unchanged columns that are not keys; neither:
    keys = all unchanged columns, targets = the added and removed columns; targets without keys raises),
    the four `df_hash_rows_on_cols` tables, the validity of keys[0] -- the first key as listed -- from
    each frame that has that column, and one `keyed_diff_digests` call. The output frame (the coalesced
    keys, the .left / .right columns, display, the status) is `diff_contents` over the returned row
    indices; `diff_dfs_contents` does both.
    The reference keeps the schema diff in HashSets, so the keys[0] of its defaulted keys is whichever
    column iteration yields first; here it is the first unchanged column in the left frame's order.
    When the keys select no column of a frame the reference joins null hashes; that case is out of
    scope here and raises OxenError."""
    left, right = _as_frame(left), _as_frame(right)
    keys, targets = _keys_targets_smart_defaults(left, right, keys, targets)
    left_keys = df_hash_rows_on_cols(left, keys, ctx=ctx) if keys else None
    right_keys = df_hash_rows_on_cols(right, keys, ctx=ctx) if keys else None
    if left_keys is None or right_keys is None:
        raise _capi.OxenError(f"the keys {keys!r} select no column of the {'left' if left_keys is None else 'right'} frame "
                              "(the reference joins null hashes there; not supported)", _capi.OXH_ERR_INVALID)
    left_targets = df_hash_rows_on_cols(left, targets, ctx=ctx)
    right_targets = df_hash_rows_on_cols(right, targets, ctx=ctx)
    valid = [(f[keys[0]].validity, f[keys[0]].validity_bit) if keys[0] in f else None for f in (left, right)]
    return keyed_diff_digests(left_keys, right_keys, left_targets, right_targets, valid[0], valid[1], ctx=ctx)


# ---------------------------------------------------------------- take: the columns of the joined rows
STATUS_COLUMN = "_oxen_diff_status"   # constants.rs DIFF_STATUS_COL


def _take_tables(cols, plan):
    """(rows, plan words, the plan as a list, kind of each output column) of a take over `cols`. plan: one
    (a, ia, b, ib) per output column, b None for no fallback; None = a plain take of every column
    through idx0."""
    if plan is None:
        plan = [(c, 0, None, 0) for c in range(len(cols))]
    plan = [tuple(p) for p in plan]
    words = []
    for a, ia, b, ib in plan:
        if not 0 <= int(a) < len(cols) or (b is not None and not 0 <= int(b) < len(cols)):
            raise _capi.OxenError(f"a plan entry names column {a if b is None else (a, b)} of {len(cols)}", _capi.OXH_ERR_INVALID)
        words += [int(a), int(ia), _capi.OXH_TAKE_NO_COLUMN if b is None else int(b), int(ib)]
    rows = (ctypes.c_uint64 * max(len(cols), 1))(*[int(c.nrows) for c in cols])
    return rows, (ctypes.c_uint32 * max(len(words), 1))(*words), plan, [int(cols[p[0]].kind) for p in plan]


def _pointers(addresses):
    return (ctypes.c_void_p * max(len(addresses), 1))(*addresses)


def _take_sizes(kinds, nout_rows, value_bytes):
    """Per output column the bytes of (values, offsets, validity)."""
    bitmap = (nout_rows + 7) // 8
    return [(int(value_bytes[o]), (nout_rows + 1) * (4 if k == OXH_COL_BYTES32 else 8) if k in _BYTES else 0, bitmap)
            for o, k in enumerate(kinds)]


def _host_index(a) -> Optional[np.ndarray]:
    """An index array as the ABI takes it: u32, OXH_TAKE_NULL = absent. Signed arrays (KeyedDiff's
    left_rows / right_rows) say absent with a negative value."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype.kind == "i":
        a = np.where(a < 0, _capi.OXH_TAKE_NULL, a)
    return np.ascontiguousarray(a, dtype=np.uint32)


def take(columns: Sequence, idx0, idx1=None, plan=None, ctx: Optional[_capi.Context] = None) -> list:
    """oxh_take_columns_host: the take (gather by row index) of `Column`s in host memory. idx0 / idx1: row
    indices, u32 with OXH_TAKE_NULL or signed with a negative value for an absent row (a null cell);
    either may be None (all absent). plan: one (a, ia, b, ib) per output column -- the cell of column a at
    idx[ia][i] when that row is present and the cell valid, else the cell of column b (None: no fallback,
    else a column of the same kind) at idx[ib][i], else null: polars' `coalesce`. None: every column through
    idx0. The columns may differ in height. Returns the output `Column`s over fresh numpy buffers that
    start at bit / offset 0, validity always present, null cells and pad bits 0: the sizes-only call, the
    allocation, then the call that writes."""
    cols = [c if isinstance(c, Column) else column(c) for c in columns]
    i0, i1 = _host_index(idx0), _host_index(idx1)
    if i0 is None and i1 is None:
        raise _capi.OxenError("take needs at least one index array", _capi.OXH_ERR_INVALID)
    if i0 is not None and i1 is not None and i0.shape != i1.shape:
        raise _capi.OxenError("the two index arrays have one length", _capi.OXH_ERR_INVALID)
    nout_rows = int((i0 if i0 is not None else i1).size)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    rows, words, plan, kinds = _take_tables(cols, plan)
    nout = len(plan)
    tables = _tables(cols, ptr)
    value_bytes = (ctypes.c_uint64 * max(nout, 1))()
    written = ctypes.c_uint32(0)
    handle, L = _handle(ctx), _capi.lib()
    head = (handle, len(cols), *tables, rows, nout_rows, ptr(i0), ptr(i1), nout, words)
    _capi.check(L.oxh_take_columns_host(*head, None, None, None, None, value_bytes, ctypes.byref(written)), "oxh_take_columns_host")
    outs = [[np.zeros(size, dtype=np.uint8) for size in sizes] for sizes in _take_sizes(kinds, nout_rows, value_bytes)]
    capacity = (ctypes.c_uint64 * max(nout, 1))(*[o[0].size for o in outs])
    arrays = [_pointers([o[k].ctypes.data if o[k].size else None for o in outs]) for k in range(3)]
    _capi.check(L.oxh_take_columns_host(*head, capacity, *arrays, value_bytes, ctypes.byref(written)), "oxh_take_columns_host")
    if nout and not written.value:
        raise _capi.OxenError("oxh_take_columns_host: the columns changed between the two calls", _capi.OXH_ERR_INVALID)
    result = []
    for (a, *_), kind, (values, offsets, validity) in zip(plan, kinds, outs):
        src = cols[a].values
        if kind in _WIDTH and getattr(src, "dtype", None) is not None and src.dtype.itemsize == _WIDTH[kind]:
            values = values.view(src.dtype)   # a Column carries a width; the source's dtype is the likeliest reading
        offs = offsets.view(np.int32 if kind == OXH_COL_BYTES32 else np.int64) if kind in _BYTES else None
        result.append(Column(kind, nout_rows, values, offs, validity, 0, 0))
    return result


def take_device(columns: Sequence[Column], idx0, idx1=None, plan=None, stream=None, ctx: Optional[_capi.Context] = None) -> list:
    """oxh_take_columns_device: `take` over `Column`s whose values / offsets / validity are torch tensors
    on the device, with idx0 / idx1 as 32-bit device tensors holding the u32 words (the left_rows /
    right_rows of `keyed_diff_digests_device` as they are: -1 is OXH_TAKE_NULL). Nothing crosses the link
    but the sizes. Returns `Column`s over fresh device tensors. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    cols = list(columns)
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None] + [t for t in (idx0, idx1) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column and index tensors must be contiguous", _capi.OXH_ERR_INVALID)
    if idx0 is None and idx1 is None:
        raise _capi.OxenError("take needs at least one index array", _capi.OXH_ERR_INVALID)
    for t in (idx0, idx1):
        if t is not None and (t.element_size() != 4 or t.dim() != 1):
            raise _capi.OxenError("index arrays are one-dimensional 32-bit tensors", _capi.OXH_ERR_INVALID)
    if idx0 is not None and idx1 is not None and idx0.numel() != idx1.numel():
        raise _capi.OxenError("the two index arrays have one length", _capi.OXH_ERR_INVALID)
    first = idx0 if idx0 is not None else idx1
    nout_rows, device = int(first.numel()), first.device
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    rows, words, plan, kinds = _take_tables(cols, plan)
    nout = len(plan)
    tables = _tables(cols, ptr)
    value_bytes = (ctypes.c_uint64 * max(nout, 1))()
    written = ctypes.c_uint32(0)
    handle, L, st = _handle(ctx), _capi.lib(), _stream(stream)
    head = (handle, len(cols), *tables, rows, nout_rows, ptr(idx0), ptr(idx1), nout, words)
    _capi.check(L.oxh_take_columns_device(*head, None, None, None, None, value_bytes, ctypes.byref(written), st),
                "oxh_take_columns_device")
    # fresh allocations are aligned far beyond the 8 bytes the bit-packed outputs need; not zero-filled: the
    # call writes every byte, and a fill queued on torch's stream is not ordered with the call's stream
    outs = [[torch.empty(size, dtype=torch.uint8, device=device) for size in sizes]
            for sizes in _take_sizes(kinds, nout_rows, value_bytes)]
    capacity = (ctypes.c_uint64 * max(nout, 1))(*[o[0].numel() for o in outs])
    arrays = [_pointers([ptr(o[k]) for o in outs]) for k in range(3)]
    _capi.check(L.oxh_take_columns_device(*head, capacity, *arrays, value_bytes, ctypes.byref(written), st),
                "oxh_take_columns_device")
    if nout and not written.value:
        raise _capi.OxenError("oxh_take_columns_device: the columns changed between the two calls", _capi.OXH_ERR_INVALID)
    result = []
    for (a, *_), kind, (values, offsets, validity) in zip(plan, kinds, outs):
        src = cols[a].values
        if kind in _WIDTH and src is not None and src.element_size() == _WIDTH[kind]:
            values = values.view(src.dtype)
        offs = offsets.view(torch.int32 if kind == OXH_COL_BYTES32 else torch.int64) if kind in _BYTES else None
        result.append(Column(kind, nout_rows, values, offs, validity, 0, 0))
    return result


def _trim_suffix(name: str, suffix: str) -> str:
    while name.endswith(suffix):   # str::trim_end_matches strips every repetition
        name = name[:-len(suffix)]
    return name


def output_columns(left: Mapping, right: Mapping, keys: Sequence[str], targets: Sequence[str], display: Sequence[str] = ()) -> list:
    """The columns of TabularDiff.contents and where each comes from: (name, (side, column), fallback)
    with side "left" / "right" and fallback None or another (side, column); the status column is not in
    the list. join_diff.rs:204-278 `get_output_columns` restated as written, with diffs.rs:975-1007
    `get_display_smart_defaults` for an empty display. keys and targets are the resolved ones (after
    `get_keys_targets_smart_defaults`).

    `order_columns_by_schema` keeps only the names that are literally columns of the RIGHT frame and
    sorts them by its schema. So a key or target the right frame lacks is dropped, and a display name
    such as "note.left" -- every name the smart defaults make has such a suffix -- survives only when the
    right frame has a column of that literal name. That is the reference's behaviour and is kept.
    A key is `coalesce(key.right, key.left)` (:95-102); where the left frame lacks the key it is the
    right column alone."""
    added, removed, unchanged = _schema_diff(left, right)
    keys, targets, display = list(keys), list(targets), list(display)
    if not display:
        for c in unchanged:
            if c not in keys and c not in targets:
                display += [c + ".left", c + ".right"]
        display += [c + ".left" for c in removed if c not in keys and c not in targets]
        display += [c + ".right" for c in added if c not in keys and c not in targets]
    position = {name: i for i, name in enumerate(right)}
    ordered = lambda names: sorted((n for n in names if n in position), key=position.get)  # noqa: E731  (a stable sort, as sort_by_key)
    out = []
    for key in ordered(keys):
        out.append((key, ("right", key), ("left", key) if key in left else None))
    for target in ordered(targets):
        if target in added:
            out.append((target + ".right", ("right", target), None))
        elif target in removed:
            out.append((target + ".left", ("left", target), None))
        else:
            out.append((target + ".left", ("left", target), None))
            out.append((target + ".right", ("right", target), None))
    for col in ordered(display):
        if col.endswith(".left"):
            stripped = _trim_suffix(col, ".left")
            if stripped in removed or stripped in unchanged:
                out.append((col, ("left", stripped), None))
        if col.endswith(".right"):
            stripped = _trim_suffix(col, ".right")
            if stripped in added or stripped in unchanged:
                out.append((col, ("right", stripped), None))
    return out


def _sort_key_plan(left: Mapping, right: Mapping, names: Sequence[str]) -> list:
    """The take plan of the sort keys of a keyed diff's contents over the sources [left columns..., right
    columns...]: every name as `coalesce(name.right, name.left)` (join_diff.rs:95-102), the side a frame
    lacks left out."""
    where = {("left", name): i for i, name in enumerate(left)}
    where.update({("right", name): len(left) + i for i, name in enumerate(right)})
    plan = []
    for name in names:
        if name in right:
            plan.append((where["right", name], 1, where["left", name] if name in left else None, 0))
        elif name in left:
            plan.append((where["left", name], 0, None, 0))
        else:
            raise _capi.OxenError(f"sort key {name!r} is a column of neither frame", _capi.OXH_ERR_INVALID)
    return plan


def _sort_names(sort, keys) -> list:
    names = list(keys) if sort is True else list(sort)
    if not names:
        raise _capi.OxenError("sort needs at least one key column", _capi.OXH_ERR_INVALID)
    return names


def _sort_orders_for(names, orders):
    """orders of `diff_contents`: None, a sequence parallel to the sort keys, or {name: order class}."""
    if orders is None or not isinstance(orders, Mapping):
        return orders
    return [orders.get(name) for name in names]


def diff_contents(left: Mapping, right: Mapping, diff: KeyedDiff, keys: Sequence[str], targets: Sequence[str],
                  display: Sequence[str] = (), ctx: Optional[_capi.Context] = None, sort=False, orders=None):
    """TabularDiff.contents of join_diff.rs `diff` after `diff_dfs`, as an ordered {name: Column}: the
    columns `output_columns` lists -- one `take` over both frames' columns through diff.left_rows /
    diff.right_rows, the keys coalesced right-then-left -- and `_oxen_diff_status`, a string column built
    from STATUS_NAMES on the host. keys / targets: the resolved ones (`diff_dfs_contents` passes them).

    sort=False (the default): the rows come in the keyed diff's canonical order and the contents are returned.
    sort=True applies `sort_df_on_keys` (join_diff.rs:107, :146-163) on every key, in the order `keys` lists
    them; a list of names sorts on those keys. The order is this project's stable one (`sort_indices`):
    ascending, nulls first, rows with equal keys in the canonical order -- one of the results the
    reference's unstable sort may produce. The sort keys are the keys' `coalesce(right, left)` columns, one
    take of just those, whether or not the output keeps them (the reference sorts before its `select`); the
    permutation is applied to left_rows, right_rows and status, and the one take of the wide columns then
    writes the contents in order. Returns (the KeyedDiff with the permuted rows, contents) so that status
    and contents stay aligned. orders: the order class of each sort key (a sequence, or {name: class}); None
    reads it from the columns' dtypes, which frames from `columns_from_arrow` do not carry
    (`sort_orders_from_arrow`)."""
    left, right = _as_frame(left), _as_frame(right)
    wanted = output_columns(left, right, keys, targets, display)
    sources = list(left.values()) + list(right.values())
    where = {("left", name): i for i, name in enumerate(left)}
    where.update({("right", name): len(left) + i for i, name in enumerate(right)})
    side = {"left": 0, "right": 1}
    plan = [(where[a], side[a[0]], None if b is None else where[b], 0 if b is None else side[b[0]]) for _, a, b in wanted]
    left_rows, right_rows = np.asarray(diff.left_rows), np.asarray(diff.right_rows)
    if sort is not False and sort is not None:
        names = _sort_names(sort, keys)
        key_columns = take(sources, left_rows, right_rows, _sort_key_plan(left, right, names), ctx=ctx)
        perm, _ = sort_indices(key_columns, _sort_orders_for(names, orders), ctx=ctx)
        left_rows, right_rows = left_rows[perm], right_rows[perm]
        diff = diff._replace(left_rows=left_rows, right_rows=right_rows, status=np.asarray(diff.status)[perm])
    taken = take(sources, left_rows, right_rows, plan, ctx=ctx) if plan else []
    contents = {name: col for (name, _, _), col in zip(wanted, taken)}
    contents[STATUS_COLUMN] = _status_column(np.asarray(diff.status))
    if sort is not False and sort is not None:
        return diff, contents
    return contents


def sort_diff_rows_device(left: Mapping, right: Mapping, diff: KeyedDiff, names: Sequence[str], orders=None, stream=None,
                          ctx: Optional[_capi.Context] = None) -> KeyedDiff:
    """The device steps of `diff_contents(sort=...)` over frames whose Columns hold device tensors and a
    KeyedDiff from `keyed_diff_digests_device`: one `take_device` of the sort keys' coalesced columns,
    `sort_indices_device`, and one `take_device` of left_rows, right_rows and status -- three fixed-width
    columns -- through the permutation. Returns the KeyedDiff with the permuted rows (device tensors); a
    `take_device` of the wide columns through them writes the contents in order. Blocks."""
    names = list(names)
    sources = list(left.values()) + list(right.values())
    key_columns = take_device(sources, diff.left_rows, diff.right_rows, _sort_key_plan(left, right, names), stream=stream, ctx=ctx)
    perm, _ = sort_indices_device(key_columns, _sort_orders_for(names, orders), stream=stream, ctx=ctx)
    n = int(perm.numel())
    rows = [Column(OXH_COL_FIXED4, n, diff.left_rows), Column(OXH_COL_FIXED4, n, diff.right_rows),
            Column(OXH_COL_FIXED1, n, diff.status)]
    l, r, s = take_device(rows, perm, stream=stream, ctx=ctx)
    return diff._replace(left_rows=l.values, right_rows=r.values, status=s.values)


def _status_column(status: np.ndarray) -> Column:
    """The string column of STATUS_NAMES[status[i]], built without a Python loop over the rows."""
    names = [name.encode() for name in STATUS_NAMES]
    table = np.frombuffer(b"".join(names), dtype=np.uint8)
    name_len = np.array([len(name) for name in names], dtype=np.int64)
    name_at = np.cumsum(name_len) - name_len
    s = status.astype(np.int64)
    lens = name_len[s]
    offsets = np.zeros(s.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    within = np.arange(int(offsets[-1]), dtype=np.int64) - np.repeat(offsets[:-1], lens)
    values = table[np.repeat(name_at[s], lens) + within]
    wide = int(offsets[-1]) > np.iinfo(np.int32).max
    return Column(OXH_COL_BYTES64 if wide else OXH_COL_BYTES32, s.size, values, offsets if wide else offsets.astype(np.int32))


def diff_dfs_contents(left: Mapping, right: Mapping, keys: Sequence[str] = (), targets: Sequence[str] = (),
                      display: Sequence[str] = (), ctx: Optional[_capi.Context] = None, sort=False, orders=None):
    """diffs.rs:881-901 `diff_dfs` with its contents: (KeyedDiff, {name: Column}) -- `diff_dfs`, then
    `diff_contents` with the keys and targets its smart defaults resolved. sort / orders: as `diff_contents`
    takes them -- False keeps the keyed diff's canonical order; True is `sort_df_on_keys` on every resolved
    key in the caller's order, a list of names on those; the KeyedDiff returned then holds the sorted rows."""
    left, right = _as_frame(left), _as_frame(right)
    resolved_keys, resolved_targets = _keys_targets_smart_defaults(left, right, keys, targets)
    d = diff_dfs(left, right, keys=keys, targets=targets, ctx=ctx)
    if sort is False or sort is None:
        return d, diff_contents(left, right, d, resolved_keys, resolved_targets, display, ctx=ctx)
    return diff_contents(left, right, d, resolved_keys, resolved_targets, display, ctx=ctx, sort=sort, orders=orders)


# ---------------------------------------------------------------- stable multi-column row sort
class SortStats(NamedTuple):
    """stats3 of oxh_sort_rows_*: refinement rounds run, radix passes launched, rows that equal another row
    on every key."""
    rounds: int
    passes: int
    tied: int


def _order_of(c: Column, k: int) -> int:
    """The default order class of key column k from the dtype of its values. A Column carries a width, not a
    dtype: raw uint8 storage (what `columns_from_arrow` makes) says nothing, and the call needs `orders`."""
    if c.kind not in _WIDTH:
        return OXH_SORT_SIGNED   # ignored for booleans and byte columns
    dt = getattr(c.values, "dtype", None)
    size = getattr(dt, "itemsize", None)
    if isinstance(dt, np.dtype):
        kind = dt.kind
    elif dt is not None:   # a torch dtype
        kind = "f" if dt.is_floating_point else ("i" if dt.is_signed else "u")
    else:
        kind = None
    if kind is None or size != _WIDTH[c.kind] or (kind == "u" and size == 1) or kind not in "fiuM":
        raise _capi.OxenError(f"sort key column {k} holds raw {dt} storage of a {_WIDTH[c.kind]}-byte cell: its dtype does not say "
                              "how it is ordered; pass orders (OXH_SORT_SIGNED / OXH_SORT_UNSIGNED / OXH_SORT_FLOAT, "
                              "sort_orders_from_arrow)", _capi.OXH_ERR_INVALID)
    return {"f": OXH_SORT_FLOAT, "i": OXH_SORT_SIGNED, "M": OXH_SORT_SIGNED, "u": OXH_SORT_UNSIGNED}[kind]


def _orders(cols, orders):
    if orders is None:
        orders = [None] * len(cols)
    orders = list(orders)
    if len(orders) != len(cols):
        raise _capi.OxenError("orders has one entry per key column", _capi.OXH_ERR_INVALID)
    words = [_order_of(c, k) if o is None else int(o) for k, (c, o) in enumerate(zip(cols, orders))]
    return (ctypes.c_uint32 * max(len(words), 1))(*words)


def sort_orders_from_arrow(schema, names) -> list:
    """The order classes of the key columns `names` of a frame made by `columns_from_arrow`, from the pyarrow
    schema: floats OXH_SORT_FLOAT, unsigned integers OXH_SORT_UNSIGNED, everything else OXH_SORT_SIGNED
    (signed integers and timestamps; booleans, strings and binary ignore theirs)."""
    import pyarrow as pa

    out = []
    for name in names:
        t = schema.field(name).type
        out.append(OXH_SORT_FLOAT if pa.types.is_floating(t) else OXH_SORT_UNSIGNED if pa.types.is_unsigned_integer(t)
                   else OXH_SORT_SIGNED)
    return out


def sort_indices(columns: Sequence, orders=None, ctx: Optional[_capi.Context] = None):
    """oxh_sort_rows_host: (perm, SortStats) -- perm[i] (uint32) = the row of the frame that stands at place i
    when its rows are sorted on `columns` (key `Column`s, or what `column` takes, most significant first, in
    host memory): ascending, a null before every value, -0.0 equal to +0.0, every NaN equal and last, byte
    columns in unsigned byte order with a proper prefix first, rows equal on every key in input order (the
    sort is stable). perm is usable as idx0 of `take`. orders: one OXH_SORT_* per key (None entries, or None
    for all: from the dtype of `values` -- float, signed integer / datetime64, unsigned integer)."""
    cols = _as_columns(columns)
    nrows = cols[0].nrows if cols else 0
    order_words = _orders(cols, orders)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    perm = np.zeros(nrows, dtype=np.uint32)
    stats = np.zeros(3, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_sort_rows_host(_handle(ctx), nrows, len(cols), *_tables(cols, ptr), order_words,
                                               perm.ctypes.data if nrows else None, stats.ctypes.data_as(_capi._u64p)),
                "oxh_sort_rows_host")
    return perm, SortStats(*(int(s) for s in stats))


def sort_indices_device(columns: Sequence[Column], orders=None, stream=None, ctx: Optional[_capi.Context] = None):
    """oxh_sort_rows_device: `sort_indices` over `Column`s whose values / offsets / validity are torch tensors
    on the device; (perm, SortStats) with perm an int32 device tensor holding the u32 words, as `take_device`
    takes its indices. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    cols = list(columns)
    nrows = cols[0].nrows if cols else 0
    if any(c.nrows != nrows for c in cols):
        raise _capi.OxenError("the columns of a frame have one row count", _capi.OXH_ERR_INVALID)
    order_words = _orders(cols, orders)
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    perm = torch.empty(nrows, dtype=torch.int32, device=device)
    stats = np.zeros(3, dtype=np.uint64)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    _capi.check(_capi.lib().oxh_sort_rows_device(_handle(ctx), nrows, len(cols), *_tables(cols, ptr), order_words,
                                                 perm.data_ptr() if nrows else None, stats.ctypes.data_as(_capi._u64p),
                                                 _stream(stream)), "oxh_sort_rows_device")
    return perm, SortStats(*(int(s) for s in stats))


def sort_by(frame: Mapping, name: str, orders=None, ctx: Optional[_capi.Context] = None) -> dict:
    """`oxen df --sort name` (core/df/tabular.rs:520-522): the frame with its rows sorted on column `name`,
    as an ordered {name: Column} -- `sort_indices` of that column, then one `take` of every column through
    the permutation. orders: the key's order class (or a one-entry sequence); None reads the dtype."""
    frame = _as_frame(frame)
    if name not in frame:
        raise _capi.OxenError(f"sort column {name!r} is not in the frame", _capi.OXH_ERR_INVALID)
    if orders is not None and not isinstance(orders, (list, tuple)):
        orders = [orders]
    perm, _ = sort_indices([frame[name]], orders, ctx=ctx)
    return dict(zip(frame, take(list(frame.values()), perm, ctx=ctx)))


# ---------------------------------------------------------------- rows grouped by equality on key columns
class GroupStats(NamedTuple):
    """stats4 of oxh_group_rows_*: the groups, the rows whose group has two or more rows (`is_duplicated().sum()`,
    the reference's `n_duped_rows`), the largest group, the rows whose key image took the long path."""
    groups: int
    duplicated: int
    largest: int
    long_rows: int


class RowGroups(NamedTuple):
    """The grouping of a frame's rows by equality on key columns. group[i]: the smallest row whose key equals
    row i's; count[i]: the rows of row i's group; first_idx: the rows with group[i] == i, ascending -- the
    selection of `unique(keep="first", maintain_order=True)`, usable as idx0 of `take` -- and first_count their
    groups' sizes, both of length stats.groups. uint32 (numpy), or int32 device tensors holding the u32 words."""
    group: Any
    count: Any
    first_idx: Any
    first_count: Any
    stats: GroupStats


def group_rows(columns: Sequence, orders=None, ctx: Optional[_capi.Context] = None) -> RowGroups:
    """oxh_group_rows_host over key `Column`s (or what `column` takes) in host memory. Rows are equal when they
    are equal in every key column: a null equals a null and nothing else, "" is not null, fixed-width cells by
    their bytes -- under OXH_SORT_FLOAT -0.0 equals +0.0 and every NaN every NaN --, byte cells by length and
    bytes (polars' documented `unique` / `group_by` behaviour, not pinned by a run of polars). orders: as
    `sort_indices` takes them (None: from the dtype of `values`); only OXH_SORT_FLOAT changes the result."""
    cols = _as_columns(columns)
    nrows = cols[0].nrows if cols else 0
    order_words = _orders(cols, orders)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    outs = [np.zeros(nrows, dtype=np.uint32) for _ in range(4)]
    stats = np.zeros(4, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_group_rows_host(_handle(ctx), nrows, len(cols), *_tables(cols, ptr), order_words,
                                                *[o.ctypes.data if nrows else None for o in outs],
                                                stats.ctypes.data_as(_capi._u64p)), "oxh_group_rows_host")
    s = GroupStats(*(int(x) for x in stats))
    return RowGroups(outs[0], outs[1], outs[2][:s.groups], outs[3][:s.groups], s)


def group_rows_device(columns: Sequence[Column], orders=None, stream=None, ctx: Optional[_capi.Context] = None) -> RowGroups:
    """oxh_group_rows_device: `group_rows` over `Column`s whose values / offsets / validity are torch tensors on
    the device; the four arrays are int32 device tensors holding the u32 words, first_idx / first_count views of
    length stats.groups (first_idx as `take_device` takes its indices). Blocks."""
    import torch

    from .device import _require_cuda, _stream

    cols = list(columns)
    nrows = cols[0].nrows if cols else 0
    if any(c.nrows != nrows for c in cols):
        raise _capi.OxenError("the columns of a frame have one row count", _capi.OXH_ERR_INVALID)
    order_words = _orders(cols, orders)
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    outs = [torch.empty(nrows, dtype=torch.int32, device=device) for _ in range(4)]
    stats = np.zeros(4, dtype=np.uint64)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    _capi.check(_capi.lib().oxh_group_rows_device(_handle(ctx), nrows, len(cols), *_tables(cols, ptr), order_words,
                                                  *[ptr(o) for o in outs], stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                "oxh_group_rows_device")
    s = GroupStats(*(int(x) for x in stats))
    return RowGroups(outs[0], outs[1], outs[2][:s.groups], outs[3][:s.groups], s)


def _key_columns(frame: Mapping, columns) -> tuple:
    frame = _as_frame(frame)
    names = [columns] if isinstance(columns, str) else list(columns)
    if not names:
        raise _capi.OxenError("grouping needs at least one key column", _capi.OXH_ERR_INVALID)
    for name in names:
        if name not in frame:
            raise _capi.OxenError(f"key column {name!r} is not in the frame", _capi.OXH_ERR_INVALID)
    return frame, names


def unique(frame: Mapping, columns, ctx: Optional[_capi.Context] = None, orders=None) -> dict:
    """`oxen df --unique columns` (core/df/tabular.rs:424-427 `unique_df`): every column of the frame at the
    first row of each distinct key, the first occurrences in input order -- `group_rows` of the named columns,
    then one `take` through first_idx. columns: a name or a list of names. orders: None (from the dtypes), a
    sequence parallel to `columns`, or {name: order class}."""
    frame, names = _key_columns(frame, columns)
    g = group_rows([frame[name] for name in names], _sort_orders_for(names, orders), ctx=ctx)
    return dict(zip(frame, take(list(frame.values()), g.first_idx, ctx=ctx)))


def unique_count(frame: Mapping, columns, ctx: Optional[_capi.Context] = None, orders=None) -> dict:
    """`oxen df --unique_count columns` (core/df/tabular.rs:429-433 `unique_count_df`): the named columns at the
    first row of each distinct key, plus `count`, the rows of that key -- UInt32 (OXH_COL_FIXED4), as polars'
    `len()` is. The groups come in the order of their first rows (the reference's order is unspecified)."""
    frame, names = _key_columns(frame, columns)
    g = group_rows([frame[name] for name in names], _sort_orders_for(names, orders), ctx=ctx)
    out = dict(zip(names, take([frame[name] for name in names], g.first_idx, ctx=ctx)))
    out["count"] = Column(OXH_COL_FIXED4, g.stats.groups, np.ascontiguousarray(g.first_count, dtype=np.uint32))
    return out


def is_duplicated(frame: Mapping, columns, ctx: Optional[_capi.Context] = None, orders=None) -> np.ndarray:
    """polars' `select(columns).is_duplicated()`: a boolean per row, True where another row has the same key."""
    frame, names = _key_columns(frame, columns)
    return group_rows([frame[name] for name in names], _sort_orders_for(names, orders), ctx=ctx).count > 1


def n_duped_rows(frame: Mapping, columns, ctx: Optional[_capi.Context] = None, orders=None) -> int:
    """core/df/tabular.rs:263-271 `n_duped_rows`: `select(columns).is_duplicated().sum()`."""
    frame, names = _key_columns(frame, columns)
    return group_rows([frame[name] for name in names], _sort_orders_for(names, orders), ctx=ctx).stats.duplicated


# ---------------------------------------------------------------- row filter: `oxen df --filter`
FILTER_OPS = {"==": _capi.OXH_FILTER_EQ, "!=": _capi.OXH_FILTER_NE, "<": _capi.OXH_FILTER_LT, "<=": _capi.OXH_FILTER_LE,
              ">": _capi.OXH_FILTER_GT, ">=": _capi.OXH_FILTER_GE}
FILTER_LOGICAL = {"&&": _capi.OXH_FILTER_AND, "||": _capi.OXH_FILTER_OR}
_FILTER_OP_SEARCH = ("!=", ">=", "<=", "==", ">", "<")   # filter.rs:130-137: the longer operators first
_INT_LITERAL = re.compile(r"[+-]?[0-9]+\Z")
# Rust's f64 / f32 FromStr: no underscores, no blanks; inf, infinity and nan in any letter case
_FLOAT_LITERAL = re.compile(r"[+-]?(?:inf|infinity|nan|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:e[+-]?[0-9]+)?)\Z", re.IGNORECASE)


class FilterExpr(NamedTuple):
    """A parsed `--filter`: terms = [(field, op, value)] with op one of == != < <= > >= and value still a
    string; logical = the "&&" / "||" between them, one fewer. They are folded left to right, no precedence."""
    terms: list
    logical: list


class FilterStats(NamedTuple):
    """stats2 of oxh_filter_rows_*: the selected rows, and the rows whose folded result is null (dropped)."""
    selected: int
    null_rows: int


class RowFilter(NamedTuple):
    """The rows a filter selects. idx: those rows, ascending, of length stats.selected, usable as idx0 of `take`
    (uint32 numpy, or an int32 device tensor holding the u32 words); mask: an Arrow bitmap of them, LSB first,
    8 * ceil(nrows / 64) bytes with the bits past nrows zero, usable as a boolean column's values (uint8). Either
    is None when it was not asked for."""
    idx: Any
    mask: Any
    stats: FilterStats


def parse_filter(expr: str) -> FilterExpr:
    """core/df/filter.rs:97-158 `parse`, restated: split at the earliest "&&" / "||" again and again, trim every
    sub-expression, look in it for the operators in the order != >= <= == > < by containment, split on the first
    one found, trim, and take parts 0 and 1 as field and value. An empty string is an error, as there; so is a
    sub-expression without an operator, which the reference drops and then panics on."""
    if not isinstance(expr, str) or expr == "":
        raise _capi.OxenError(f"cannot parse the filter {expr!r}", _capi.OXH_ERR_INVALID)
    rest, subs, logical = expr, [], []
    while True:
        found = [(at, op) for op in ("&&", "||") for at in [rest.find(op)] if at >= 0]
        if not found:
            break
        at, op = min(found)
        subs.append(rest[:at].strip())
        logical.append(op)
        rest = rest[at + len(op):]
    subs.append(rest.strip())
    terms = []
    for sub in subs:
        op = next((o for o in _FILTER_OP_SEARCH if o in sub), None)
        if op is None:
            raise _capi.OxenError(f"the filter's sub-expression {sub!r} has no operator (== != < <= > >=)", _capi.OXH_ERR_INVALID)
        parts = [p.strip() for p in sub.split(op)]
        terms.append((parts[0], op, parts[1]))
    return FilterExpr(terms, logical)


def _round_to_f32(text: str) -> np.float32:
    """The f32 nearest to the decimal `text`, ties to even, as Rust's `f32::from_str` gives it -- not the f64
    nearest to it rounded once more."""
    from fractions import Fraction

    d = float(text)
    with np.errstate(over="ignore"):
        near = np.float32(d)
    if not np.isfinite(d) or d == 0.0:     # inf, nan, and what overflows or underflows f64 does so in f32
        return near
    exact = Fraction(text)
    top = Fraction(float(np.finfo(np.float32).max))
    if abs(exact) >= top + Fraction(2) ** 103:   # half an ulp above the largest f32: infinity
        return np.float32(np.copysign(np.inf, d))
    near = np.float32(np.copysign(float(top), d)) if np.isinf(near) else near
    best = None
    with np.errstate(over="ignore"):
        around = (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf)))
    for cand in around:
        if not np.isfinite(cand):
            continue
        key = (abs(Fraction(float(cand)) - exact), int(cand.view(np.uint32)) & 1)   # the distance, then the even mantissa
        if best is None or key < best[0]:
            best = (key, cand)
    return -abs(best[1]) if d < 0 else abs(best[1])   # a tiny value that rounds to zero keeps its sign


def _filter_literal(c: Column, order: int, value: str, what: str):
    """The literal of one term typed by its column (core/df/tabular.rs:332-361 `val_from_str_and_dtype`): an int
    (the ABI's term_word) or bytes (a byte column's literal)."""
    import struct

    def bad(expected):
        return _capi.OxenError(f"{what}: {value!r} is not {expected}", _capi.OXH_ERR_INVALID)

    if c.kind in _BYTES:
        return value.encode("utf-8")
    if c.kind == OXH_COL_BOOL:
        if value not in ("true", "false"):
            raise bad("a boolean (true / false)")
        return int(value == "true")
    width = _WIDTH[c.kind]
    if order == OXH_SORT_FLOAT:
        if not _FLOAT_LITERAL.match(value):
            raise bad("a float")
        if width == 8:
            return struct.unpack("<Q", struct.pack("<d", float(value)))[0]
        return int(_round_to_f32(value).view(np.uint32))
    if not _INT_LITERAL.match(value):
        raise bad("an integer")
    v, bits = int(value), 8 * width
    lo, hi = (0, (1 << bits) - 1) if order == OXH_SORT_UNSIGNED else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    if not lo <= v <= hi:
        raise bad(f"in the range of a{'n unsigned' if order == OXH_SORT_UNSIGNED else ' signed'} {bits}-bit column")
    return v & ((1 << bits) - 1)


def _filter_orders(cols, orders, named) -> list:
    """One order class per column: a column a term names reads its dtype where none is given (`_order_of`); the
    others are not read by the call and default to OXH_SORT_SIGNED."""
    orders = [None] * len(cols) if orders is None else list(orders)
    if len(orders) != len(cols):
        raise _capi.OxenError("orders has one entry per column", _capi.OXH_ERR_INVALID)
    return [int(o) if o is not None else (_order_of(c, k) if k in named else OXH_SORT_SIGNED)
            for k, (c, o) in enumerate(zip(cols, orders))]


def filter_terms(frame: Mapping, expr, orders=None) -> tuple:
    """(terms, logical) as `filter_rows` takes them, from a `--filter` string or a `FilterExpr`: every field
    resolved to the index of its column in the frame, every literal typed by that column -- booleans exactly
    `true` / `false`; integers `[+-]?[0-9]+` that fit the column's width and signedness; floats as Rust's
    `FromStr` reads them, rounded to f32 for a 4-byte column; the UTF-8 bytes for a byte column. An unknown
    field or an unparsable literal raises OxenError (OXH_ERR_INVALID), where the reference would panic. orders:
    None (from the dtypes), a sequence parallel to the frame's columns, or {name: order class}."""
    frame = _as_frame(frame)
    parsed = expr if isinstance(expr, FilterExpr) else parse_filter(expr)
    names = list(frame)
    if len(parsed.logical) != len(parsed.terms) - 1:
        raise _capi.OxenError("a filter has one logical operator fewer than terms", _capi.OXH_ERR_INVALID)
    for field, op, _ in parsed.terms:
        if field not in frame:
            raise _capi.OxenError(f"filter field {field!r} is not in the frame", _capi.OXH_ERR_INVALID)
        if op not in FILTER_OPS:
            raise _capi.OxenError(f"unknown filter operator {op!r}", _capi.OXH_ERR_INVALID)
    for op in parsed.logical:
        if op not in FILTER_LOGICAL:
            raise _capi.OxenError(f"unknown logical operator {op!r}", _capi.OXH_ERR_INVALID)
    named = {names.index(field) for field, _, _ in parsed.terms}
    per_column = [orders.get(name) for name in names] if isinstance(orders, Mapping) else orders
    order_of = _filter_orders(list(frame.values()), per_column, named)
    terms = []
    for field, op, value in parsed.terms:
        k = names.index(field)
        terms.append((k, FILTER_OPS[op], _filter_literal(frame[field], order_of[k], value, f"filter term {field} {op} {value}")))
    return terms, [FILTER_LOGICAL[op] for op in parsed.logical]


def _filter_tables(cols, terms, logical, orders):
    """The term arrays of the ABI, and the columns' order words. terms: (column index, OXH_FILTER_* operator,
    literal) with the literal an int (term_word) or bytes; logical: OXH_FILTER_AND / OXH_FILTER_OR, one fewer."""
    terms, logical = list(terms), [int(x) for x in logical]
    if terms and len(logical) != len(terms) - 1:
        raise _capi.OxenError("a filter has one logical operator fewer than terms", _capi.OXH_ERR_INVALID)
    named = {int(t[0]) for t in terms if 0 <= int(t[0]) < len(cols)}
    order_words = (ctypes.c_uint32 * max(len(cols), 1))(*_filter_orders(cols, orders, named))
    n = len(terms)
    col = (ctypes.c_uint32 * max(n, 1))(*[int(t[0]) for t in terms])
    op = (ctypes.c_uint32 * max(n, 1))(*[int(t[1]) for t in terms])
    words = [0 if isinstance(t[2], (bytes, bytearray)) else int(t[2]) for t in terms]
    word = (ctypes.c_uint64 * max(n, 1))(*words)
    literals = [bytes(t[2]) if isinstance(t[2], (bytes, bytearray)) else b"" for t in terms]
    lit_offsets = (ctypes.c_uint64 * (n + 1))(*np.cumsum([0] + [len(b) for b in literals]).tolist())
    lit = b"".join(literals)
    lit_bytes = ctypes.create_string_buffer(lit, len(lit)) if lit else None
    log = (ctypes.c_uint32 * max(len(logical), 1))(*logical)
    return order_words, (n, col, op, word, lit_bytes, lit_offsets, log)


def filter_rows(columns: Sequence, terms, logical=(), orders=None, want_mask: bool = False, ctx: Optional[_capi.Context] = None,
                want_idx: bool = True) -> RowFilter:
    """oxh_filter_rows_host over the `Column`s of a frame (or what `column` takes) in host memory: the rows for
    which the terms `column OP literal`, folded left to right by `logical` with no precedence, give TRUE. A term
    on a null cell is null for every operator; && and || are Kleene's; null and false rows are dropped. Fixed-width
    cells compare by the sort's canonical word (OXH_SORT_FLOAT: -0.0 == +0.0, every NaN equal and above +inf),
    booleans false < true, byte cells unsigned byte-wise with a proper prefix first (polars' documented behaviour,
    not pinned by a run of polars). terms / logical: what `filter_terms` returns. orders: one OXH_SORT_* per
    column, None entries (or None) reading the dtype of a column a term names."""
    cols = _as_columns(columns)
    nrows = cols[0].nrows if cols else 0
    order_words, term_tables = _filter_tables(cols, terms, logical, orders)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    idx = np.zeros(nrows, dtype=np.uint32) if want_idx else None
    mask = np.zeros(-(-nrows // 64), dtype=np.uint64) if want_mask else None
    stats = np.zeros(2, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_filter_rows_host(_handle(ctx), nrows, len(cols), *_tables(cols, ptr), order_words, *term_tables,
                                                 idx.ctypes.data if want_idx and nrows else None,
                                                 mask.ctypes.data if want_mask and nrows else None,
                                                 stats.ctypes.data_as(_capi._u64p)), "oxh_filter_rows_host")
    s = FilterStats(*(int(x) for x in stats))
    return RowFilter(idx[:s.selected] if want_idx else None, mask.view(np.uint8) if want_mask else None, s)


def filter_rows_device(columns: Sequence[Column], terms, logical=(), orders=None, want_mask: bool = False, stream=None,
                       ctx: Optional[_capi.Context] = None, want_idx: bool = True) -> RowFilter:
    """oxh_filter_rows_device: `filter_rows` over `Column`s whose values / offsets / validity are torch tensors on
    the device; idx is a view of length stats.selected of an int32 device tensor holding the u32 words (as
    `take_device` takes its indices), mask a uint8 device tensor. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    cols = list(columns)
    nrows = cols[0].nrows if cols else 0
    if any(c.nrows != nrows for c in cols):
        raise _capi.OxenError("the columns of a frame have one row count", _capi.OXH_ERR_INVALID)
    order_words, term_tables = _filter_tables(cols, terms, logical, orders)
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    idx = torch.empty(nrows, dtype=torch.int32, device=device) if want_idx else None
    mask = torch.empty(-(-nrows // 64), dtype=torch.int64, device=device) if want_mask else None
    stats = np.zeros(2, dtype=np.uint64)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    _capi.check(_capi.lib().oxh_filter_rows_device(_handle(ctx), nrows, len(cols), *_tables(cols, ptr), order_words, *term_tables,
                                                   ptr(idx), ptr(mask), stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                "oxh_filter_rows_device")
    s = FilterStats(*(int(x) for x in stats))
    return RowFilter(idx[:s.selected] if want_idx else None, mask.view(torch.uint8) if want_mask else None, s)


def filter_df(frame: Mapping, expr, ctx: Optional[_capi.Context] = None, orders=None) -> dict:
    """`oxen df --filter expr` (core/df/tabular.rs:404-422 `filter_df`): the frame's rows for which the filter
    gives true, in input order, as an ordered {name: Column} -- `filter_terms`, `filter_rows`, then one `take` of
    every column through idx. The result feeds `unique`, `unique_count` and `sort_by` as it is. expr: a
    `--filter` string or a `FilterExpr`; orders: as `filter_terms` takes them."""
    frame = _as_frame(frame)
    names = list(frame)
    terms, logical = filter_terms(frame, expr, orders)
    per_column = [orders.get(name) for name in names] if isinstance(orders, Mapping) else orders
    selected = filter_rows(list(frame.values()), terms, logical, per_column, ctx=ctx)
    return dict(zip(frame, take(list(frame.values()), selected.idx, ctx=ctx)))


def _buffer(buf, dtype) -> Optional[np.ndarray]:
    return None if buf is None or buf.size == 0 else np.frombuffer(buf, dtype=dtype)


def _arrow_column(name, arr) -> Column:
    import pyarrow as pa

    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
    t, n, off = arr.type, len(arr), arr.offset
    bufs = arr.buffers()
    validity = _buffer(bufs[0], np.uint8) if arr.null_count else None
    vbit = off if validity is not None else 0
    width = {pa.int8(): 1, pa.int32(): 4, pa.float32(): 4, pa.int64(): 8, pa.float64(): 8}.get(t)
    if width is None and pa.types.is_timestamp(t) and t.unit == "ms":
        width = 8
    if width is not None:
        data = _buffer(bufs[1], np.uint8)
        values = data[off * width:(off + n) * width] if data is not None else np.zeros(0, dtype=np.uint8)
        return Column(width, n, values, None, validity, 0, vbit)
    if pa.types.is_boolean(t):
        return Column(OXH_COL_BOOL, n, _buffer(bufs[1], np.uint8), None, validity, off, vbit)
    for kind, odt, match in ((OXH_COL_BYTES32, np.int32, (pa.types.is_string, pa.types.is_binary)),
                             (OXH_COL_BYTES64, np.int64, (pa.types.is_large_string, pa.types.is_large_binary))):
        if any(m(t) for m in match):
            offsets = _buffer(bufs[1], odt)
            offsets = offsets[off:off + n + 1] if offsets is not None else np.zeros(n + 1, dtype=odt)
            return Column(kind, n, _buffer(bufs[2], np.uint8), offsets, validity, 0, vbit)
    raise _capi.OxenError(f"column {name!r}: Arrow type {t} has no raw row bytes in the reference (it goes through "
                          "to_string()): cast it to string first", _capi.OXH_ERR_INVALID)


def columns_from_arrow(table_or_batch) -> dict:
    """A pyarrow Table / RecordBatch as a frame: {name: Column} in schema order, the columns pointing
    into the Arrow buffers (slices keep their offsets: nothing is copied but a chunked column's chunks).
    Int8 / Int32 / Int64 / Float32 / Float64 / Timestamp(ms) / Boolean / (Large)Utf8 / (Large)Binary;
    any other type raises: cast it to string, which is what the reference's `to_string()` arm amounts to."""
    names = table_or_batch.schema.names
    return {name: _arrow_column(name, table_or_batch.column(i)) for i, name in enumerate(names)}


def columns_to_arrow(columns: Mapping, schema):
    """The inverse of `columns_from_arrow` for callers with pyarrow: a pyarrow Table over the buffers of
    {name: Column} (host memory; what `take` and `diff_contents` return). schema: a pyarrow Schema naming
    every column -- a Column carries a width, the schema says the type (int32 or float32, string or
    binary). Nothing is copied but a bitmap that does not start at bit 0 (a sliced source, never a take's
    output), which is repacked: an Arrow array has one offset for all its buffers, a Column one per bitmap."""
    import pyarrow as pa

    as_buffer = lambda a: None if a is None else pa.py_buffer(np.ascontiguousarray(a).view(np.uint8))  # noqa: E731

    def bitmap(packed, bit0, n):
        if packed is None or not bit0:
            return as_buffer(packed)
        return as_buffer(_pack(np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[bit0:bit0 + n]))

    arrays = []
    for field in schema:
        c = columns[field.name]
        n = int(c.nrows)
        validity = bitmap(c.validity, int(c.validity_bit), n)
        if c.kind == OXH_COL_BOOL:
            buffers = [validity, bitmap(c.values, int(c.value_bit), n)]
        else:
            values = as_buffer(c.values) if c.values is not None and len(c.values) else pa.py_buffer(b"")
            buffers = [validity, as_buffer(c.offsets), values] if c.kind in _BYTES else [validity, values]
        arrays.append(pa.Array.from_buffers(field.type, n, buffers))
    return pa.Table.from_arrays(arrays, schema=schema)


# ---------------------------------------------------------------- embedding similarity: mean query, cosine, ranked rows
class Embedding(NamedTuple):
    """A column of `nrows` vectors of exactly `dim` float32 values as `oxh_embedding_*` takes it (numpy arrays for
    the host forms, torch tensors on the device for the device forms). layout: OXH_EMB_FIXED (row r's floats
    start at values[r * dim]), OXH_EMB_LIST32 / OXH_EMB_LIST64 (nrows + 1 int32 / int64 offsets that count
    elements of values); values: float32, one-dimensional; validity: an Arrow validity bitmap (uint8) or None
    for no nulls -- a null row is a null vector; validity_bit: the bit of row 0 in validity."""
    layout: int
    dim: int
    nrows: int
    values: Any
    offsets: Any = None
    validity: Any = None
    validity_bit: int = 0


class EmbeddingStats(NamedTuple):
    """stats4 of oxh_embedding_*: rows used (valid and of length dim), null rows, valid rows of another length,
    the smallest such row (nrows when there is none)."""
    used: int
    null_rows: int
    wrong_length: int
    first_wrong: int


class Similarity(NamedTuple):
    """What `cosine_similarity` returns: sim (float32 per row, 0.0 for a null), validity (an Arrow bitmap from bit
    0, uint8; None when the column has no validity), order_key (uint32: the descending order as an ascending
    key), perm (uint32: the rows from the most similar on -- NaNs, then +1 .. -1, then nulls, ties in input
    order), stats. order_key and perm are None when the order was not asked for."""
    sim: Any
    validity: Any
    order_key: Any
    perm: Any
    stats: EmbeddingStats


def embedding(values_2d, validity=None) -> Embedding:
    """An Embedding in the fixed layout from an (nrows, dim) array of float32 (anything else is cast).
    validity: a boolean mask (True = present) or None."""
    a = np.ascontiguousarray(values_2d, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 1:
        raise _capi.OxenError("an embedding column is an (nrows, dim) array with dim >= 1", _capi.OXH_ERR_INVALID)
    return Embedding(_capi.OXH_EMB_FIXED, int(a.shape[1]), int(a.shape[0]), a.reshape(-1), None,
                     None if validity is None else _pack(validity), 0)


def embedding_from_arrow(array, dim: Optional[int] = None) -> Embedding:
    """An Embedding over the buffers of a pyarrow FixedSizeList / List / LargeList array of float32: sliced and
    chunked arrays included (only a chunked array's chunks are copied), the child array's own offset honoured.
    dim: the vectors' length for the list layouts (None: that of the first valid row); a valid row of another
    length is what the calls refuse. Float64 children (`get_avg_embedding`'s ExpectedF32), null elements inside
    a vector and every other type raise OxenError (OXH_ERR_INVALID)."""
    import pyarrow as pa

    if isinstance(array, pa.ChunkedArray):
        array = array.combine_chunks() if array.num_chunks != 1 else array.chunk(0)
    t, n, off = array.type, len(array), array.offset
    fixed, wide = pa.types.is_fixed_size_list(t), pa.types.is_large_list(t)
    if not (fixed or wide or pa.types.is_list(t)):
        raise _capi.OxenError(f"Arrow type {t} is not a list of float32", _capi.OXH_ERR_INVALID)
    if t.value_type != pa.float32():
        raise _capi.OxenError(f"an embedding holds float32 values, not {t.value_type} (the reference's ExpectedF32)", _capi.OXH_ERR_INVALID)
    bufs = array.buffers()
    validity = _buffer(bufs[0], np.uint8) if array.null_count else None
    vbit = off if validity is not None else 0
    child = array.values   # the whole child array, before the parent's offset
    data = _buffer(child.buffers()[1], np.float32)
    data = np.zeros(0, dtype=np.float32) if data is None else data[child.offset:child.offset + len(child)]
    present = np.ones(n, dtype=bool) if validity is None else np.unpackbits(validity, bitorder="little")[vbit:vbit + n].astype(bool)
    if fixed:
        d = int(t.list_size)
        lo, hi = off * d, (off + n) * d
        layout, offsets, values = _capi.OXH_EMB_FIXED, None, data[lo:hi]
        lengths = np.full(n, d, dtype=np.int64)
    else:
        odt = np.int64 if wide else np.int32
        offsets = _buffer(bufs[1], odt)
        offsets = offsets[off:off + n + 1] if offsets is not None else np.zeros(n + 1, dtype=odt)
        layout, values = (_capi.OXH_EMB_LIST64 if wide else _capi.OXH_EMB_LIST32), data
        lo, hi = (int(offsets[0]), int(offsets[-1])) if n else (0, 0)
        lengths = np.diff(offsets.astype(np.int64))
        d = int(dim) if dim is not None else (int(lengths[present][0]) if present.any() else 1)
    if d < 1:
        raise _capi.OxenError("an embedding has at least one element per row", _capi.OXH_ERR_INVALID)
    if child.null_count and hi > lo and child.slice(lo, hi - lo).null_count:
        # a null row's own slots may be null; an element of a valid row may not
        element_valid = child.slice(lo, hi - lo).is_valid().to_numpy(zero_copy_only=False)
        if lengths.min() < 0 or int(lengths.sum()) != hi - lo or (~element_valid & np.repeat(present, lengths)).any():
            raise _capi.OxenError("null elements inside a vector are not supported", _capi.OXH_ERR_INVALID)
    return Embedding(layout, d, n, values, offsets, validity, vbit)


def embedding_to_arrow(emb: Embedding):
    """A pyarrow FixedSizeList<float32>[dim] array over the buffers of a fixed-layout Embedding in host memory with
    its validity at bit 0 (what `embedding_take` returns)."""
    import pyarrow as pa

    if emb.layout != _capi.OXH_EMB_FIXED or emb.validity_bit:
        raise _capi.OxenError("embedding_to_arrow takes the fixed layout with validity from bit 0", _capi.OXH_ERR_INVALID)
    child = pa.Array.from_buffers(pa.float32(), emb.nrows * emb.dim, [None, pa.py_buffer(np.ascontiguousarray(emb.values, dtype=np.float32))])
    validity = None if emb.validity is None else pa.py_buffer(np.ascontiguousarray(emb.validity))
    return pa.Array.from_buffers(pa.list_(pa.float32(), emb.dim), emb.nrows, [validity], children=[child])


def _embedding_args(emb: Embedding, ptr):
    return (int(emb.layout), int(emb.nrows), int(emb.dim), ptr(emb.values), ptr(emb.offsets) if emb.layout != _capi.OXH_EMB_FIXED else None,
            ptr(emb.validity), int(emb.validity_bit))


def _host_ptr(keep):
    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None
    return ptr


def _embedding_tensors(emb: Embedding, *more):
    from .device import _require_cuda

    tensors = [t for t in (emb.values, emb.offsets, emb.validity) + more if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("embedding tensors must be contiguous", _capi.OXH_ERR_INVALID)
    return tensors[0].device if tensors else "cuda"


_device_ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731


def _no_rows(stats: EmbeddingStats):
    if stats.used == 0:
        raise _capi.OxenError("no rows found: the query selects no row with an embedding", _capi.OXH_ERR_INVALID)


def embedding_mean(emb: Embedding, idx, ctx: Optional[_capi.Context] = None):
    """oxh_embedding_mean_host: (mean, EmbeddingStats) -- the element-wise float32 mean of the rows idx (ascending
    u32 row indices: what `filter_rows` returns) of an Embedding in host memory, null rows skipped. The reference's
    `get_avg_embedding`, over ALL matching rows (it pushes only the first row of every record batch; the two
    agree where one row matches). Bit-identical from run to run and with the device form. Raises the reference's
    "no rows found" when no row is used."""
    i = np.ascontiguousarray(idx, dtype=np.uint32)
    keep = []
    ptr = _host_ptr(keep)
    out = np.zeros(emb.dim, dtype=np.float32)
    stats = np.zeros(4, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_embedding_mean_host(_handle(ctx), *_embedding_args(emb, ptr), ptr(i), i.size, out.ctypes.data,
                                                    stats.ctypes.data_as(_capi._u64p)), "oxh_embedding_mean_host")
    s = EmbeddingStats(*(int(x) for x in stats))
    _no_rows(s)
    return out, s


def embedding_mean_device(emb: Embedding, idx, stream=None, ctx: Optional[_capi.Context] = None):
    """oxh_embedding_mean_device: `embedding_mean` over an Embedding of device tensors and idx as a 32-bit device
    tensor (the idx of `filter_rows_device` as it is); the mean is a float32 device tensor. Blocks."""
    import torch

    from .device import _stream

    device = _embedding_tensors(emb, idx)
    if idx.element_size() != 4 or idx.dim() != 1:
        raise _capi.OxenError("idx is a one-dimensional 32-bit tensor", _capi.OXH_ERR_INVALID)
    out = torch.empty(emb.dim, dtype=torch.float32, device=device)
    stats = np.zeros(4, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_embedding_mean_device(_handle(ctx), *_embedding_args(emb, _device_ptr), _device_ptr(idx), idx.numel(),
                                                      out.data_ptr(), stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                "oxh_embedding_mean_device")
    s = EmbeddingStats(*(int(x) for x in stats))
    _no_rows(s)
    return out, s


def cosine_similarity(emb: Embedding, query, want_order: bool = True, ctx: Optional[_capi.Context] = None) -> Similarity:
    """oxh_embedding_similarity_host: the cosine similarity of every row of an Embedding in host memory with
    `query` (dim float32) -- dot / sqrtf(nx * nq) in float32, clamped to [-1, 1]; a zero row or query gives NaN; a
    null row a null similarity -- and, with want_order, the descending order: order_key and the stable perm (NaNs
    first, then +1 .. -1, nulls last, ties in input order). Restates DuckDB's `array_cosine_similarity` and
    `ORDER BY .. DESC`; not pinned by a run of DuckDB."""
    q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
    if q.size != emb.dim:
        raise _capi.OxenError(f"the query has {q.size} elements, the column's vectors {emb.dim}", _capi.OXH_ERR_INVALID)
    n = int(emb.nrows)
    keep = []
    ptr = _host_ptr(keep)
    sim = np.zeros(n, dtype=np.float32)
    validity = np.zeros(-(-n // 8), dtype=np.uint8) if emb.validity is not None else None
    key = np.zeros(n, dtype=np.uint32) if want_order else None
    perm = np.zeros(n, dtype=np.uint32) if want_order else None
    stats = np.zeros(4, dtype=np.uint64)
    addr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    _capi.check(_capi.lib().oxh_embedding_similarity_host(_handle(ctx), *_embedding_args(emb, ptr), ptr(q), addr(sim), addr(validity),
                                                          addr(key), addr(perm), stats.ctypes.data_as(_capi._u64p)),
                "oxh_embedding_similarity_host")
    return Similarity(sim, validity, key, perm, EmbeddingStats(*(int(x) for x in stats)))


def cosine_similarity_device(emb: Embedding, query, want_order: bool = True, stream=None, ctx: Optional[_capi.Context] = None) -> Similarity:
    """oxh_embedding_similarity_device: `cosine_similarity` over an Embedding of device tensors and a float32 device
    query; sim is a float32 device tensor, validity uint8, order_key and perm int32 tensors holding the u32 words
    (perm as `take_device` takes its indices). Blocks."""
    import torch

    from .device import _stream

    device = _embedding_tensors(emb, query)
    if query.dtype != torch.float32 or query.numel() != emb.dim:
        raise _capi.OxenError(f"the query is {emb.dim} float32 values", _capi.OXH_ERR_INVALID)
    n = int(emb.nrows)
    sim = torch.empty(n, dtype=torch.float32, device=device)
    validity = torch.empty(-(-n // 8), dtype=torch.uint8, device=device) if emb.validity is not None else None
    key = torch.empty(n, dtype=torch.int32, device=device) if want_order else None
    perm = torch.empty(n, dtype=torch.int32, device=device) if want_order else None
    stats = np.zeros(4, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_embedding_similarity_device(_handle(ctx), *_embedding_args(emb, _device_ptr), _device_ptr(query),
                                                            _device_ptr(sim), _device_ptr(validity), _device_ptr(key), _device_ptr(perm),
                                                            stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                "oxh_embedding_similarity_device")
    return Similarity(sim, validity, key, perm, EmbeddingStats(*(int(x) for x in stats)))


def embedding_take(emb: Embedding, idx, ctx: Optional[_capi.Context] = None) -> Embedding:
    """oxh_embedding_take_host: the rows idx (u32 with OXH_TAKE_NULL, or signed with a negative value, for an absent
    row) of an Embedding in host memory as a fresh Embedding in the fixed layout, validity always present from bit
    0; an absent index and a null source row give zeros and a null."""
    i = _host_index(idx)
    keep = []
    ptr = _host_ptr(keep)
    values = np.zeros(i.size * emb.dim, dtype=np.float32)
    validity = np.zeros(-(-i.size // 8), dtype=np.uint8)
    stats = np.zeros(4, dtype=np.uint64)
    addr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    _capi.check(_capi.lib().oxh_embedding_take_host(_handle(ctx), *_embedding_args(emb, ptr), ptr(i), i.size, addr(values), addr(validity),
                                                    stats.ctypes.data_as(_capi._u64p)), "oxh_embedding_take_host")
    return Embedding(_capi.OXH_EMB_FIXED, emb.dim, int(i.size), values, None, validity, 0)


def embedding_take_device(emb: Embedding, idx, stream=None, ctx: Optional[_capi.Context] = None) -> Embedding:
    """oxh_embedding_take_device: `embedding_take` over an Embedding of device tensors and idx as a 32-bit device
    tensor holding the u32 words (-1 is OXH_TAKE_NULL); a fixed-layout Embedding over fresh device tensors. Blocks."""
    import torch

    from .device import _stream

    device = _embedding_tensors(emb, idx)
    if idx.element_size() != 4 or idx.dim() != 1:
        raise _capi.OxenError("idx is a one-dimensional 32-bit tensor", _capi.OXH_ERR_INVALID)
    n = int(idx.numel())
    values = torch.empty(n * emb.dim, dtype=torch.float32, device=device)
    validity = torch.empty(-(-n // 8), dtype=torch.uint8, device=device)
    stats = np.zeros(4, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_embedding_take_device(_handle(ctx), *_embedding_args(emb, _device_ptr), _device_ptr(idx), n, _device_ptr(values),
                                                      _device_ptr(validity), stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                "oxh_embedding_take_device")
    return Embedding(_capi.OXH_EMB_FIXED, emb.dim, n, values, None, validity, 0)


def page_rows(nrows: int, page_size: int, page_num: int = 1) -> tuple:
    """(first, count) of `LIMIT page_size OFFSET (page_num - 1) * page_size` over nrows ranked rows, clipped to the
    frame; page_num 0 means 1 (embeddings.rs `nearest_neighbors`)."""
    nrows, page_size, page_num = int(nrows), int(page_size), int(page_num)
    if nrows < 0 or page_size < 0 or page_num < 0:
        raise _capi.OxenError("nrows, page_size and page_num are not negative", _capi.OXH_ERR_INVALID)
    first = min((max(page_num, 1) - 1) * page_size, nrows)
    return first, min(page_size, nrows - first)


def _check_frame_rows(frame, emb):
    for name, c in frame.items():
        if c.nrows != emb.nrows:
            raise _capi.OxenError(f"column {name!r} has {c.nrows} rows, the embedding column {emb.nrows}", _capi.OXH_ERR_INVALID)


def nearest_neighbors(frame: Mapping, emb: Embedding, query, page_size: int, page_num: int = 1, name: str = "similarity",
                      ctx: Optional[_capi.Context] = None, embedding_name: str = "embedding") -> dict:
    """embeddings.rs `nearest_neighbors` (:413-567) over a frame and its embedding column in host memory: the
    similarity of every row with `query`, the rows ranked from the most similar on, and page `page_num` of
    `page_size` rows (0 means 1; clipped to the frame) as an ordered dict -- the frame's columns through `take`,
    `embedding_name`: the page's own vectors (`embedding_take`, a fixed-layout Embedding), and `name`: a float32
    Column with its validity."""
    frame = _as_frame(frame)
    _check_frame_rows(frame, emb)
    ranked = cosine_similarity(emb, query, ctx=ctx)
    first, count = page_rows(emb.nrows, page_size, page_num)
    rows = ranked.perm[first:first + count]
    sim = Column(OXH_COL_FIXED4, emb.nrows, ranked.sim, None, ranked.validity, 0, 0)
    taken = take(list(frame.values()) + [sim], rows, ctx=ctx)
    page = dict(zip(frame, taken))
    page[embedding_name] = embedding_take(emb, rows, ctx=ctx)
    page[name] = taken[-1]
    return page


def nearest_neighbors_device(frame: Mapping, emb: Embedding, query, page_size: int, page_num: int = 1, name: str = "similarity",
                             stream=None, ctx: Optional[_capi.Context] = None, embedding_name: str = "embedding") -> dict:
    """`nearest_neighbors` over device tensors: similarity, the sort, the page's rows (a view of perm), the take of
    the columns and of the vectors all stay on the device; only counts and sizes cross the link. Blocks."""
    frame = dict(frame)
    _check_frame_rows(frame, emb)
    ranked = cosine_similarity_device(emb, query, stream=stream, ctx=ctx)
    first, count = page_rows(emb.nrows, page_size, page_num)
    rows = ranked.perm[first:first + count]
    sim = Column(OXH_COL_FIXED4, emb.nrows, ranked.sim, None, ranked.validity, 0, 0)
    taken = take_device(list(frame.values()) + [sim], rows, stream=stream, ctx=ctx)
    page = dict(zip(frame, taken))
    page[embedding_name] = embedding_take_device(emb, rows, stream=stream, ctx=ctx)
    page[name] = taken[-1]
    return page


def sort_by_similarity(frame: Mapping, emb: Embedding, where, page_size: int, page_num: int = 1, name: str = "similarity",
                       ctx: Optional[_capi.Context] = None, orders=None, embedding_name: str = "embedding") -> dict:
    """embeddings.rs `query` (`oxen df --find-embedding-where where --sort-by-similarity-to column`): the rows `where`
    selects, the mean of their vectors, then `nearest_neighbors` of that mean. Two differences from the reference:
    `where` is this project's `--filter` grammar (`filter_terms`: `id == 42`, `label == dog && score > 0.5`), not
    SQL; and the mean is over ALL the selected rows, where the reference's `get_avg_embedding` takes only the
    first row of every record batch (its comment and name say average) -- the two agree where one row matches.
    Raises "no rows found" when the clause selects no row with an embedding."""
    frame = _as_frame(frame)
    _check_frame_rows(frame, emb)
    terms, logical = filter_terms(frame, where, orders)
    per_column = [orders.get(n) for n in frame] if isinstance(orders, Mapping) else orders
    selected = filter_rows(list(frame.values()), terms, logical, per_column, ctx=ctx)
    mean, _ = embedding_mean(emb, selected.idx, ctx=ctx)
    return nearest_neighbors(frame, emb, mean, page_size, page_num, name, ctx=ctx, embedding_name=embedding_name)


def sort_by_similarity_device(frame: Mapping, emb: Embedding, where, page_size: int, page_num: int = 1, name: str = "similarity",
                              stream=None, ctx: Optional[_capi.Context] = None, orders=None, embedding_name: str = "embedding") -> dict:
    """`sort_by_similarity` over device tensors: the filter's idx, the mean, the similarities, the permutation and
    the page stay on the device from end to end; nothing row-shaped is copied to the host. Blocks."""
    frame = dict(frame)
    _check_frame_rows(frame, emb)
    terms, logical = filter_terms(frame, where, orders)
    per_column = [orders.get(n) for n in frame] if isinstance(orders, Mapping) else orders
    selected = filter_rows_device(list(frame.values()), terms, logical, per_column, stream=stream, ctx=ctx)
    mean, _ = embedding_mean_device(emb, selected.idx, stream=stream, ctx=ctx)
    return nearest_neighbors_device(frame, emb, mean, page_size, page_num, name, stream=stream, ctx=ctx, embedding_name=embedding_name)


# ---------------------------------------------------------------- concat: vstack, slice, head, tail, page
_SLICE_NUMBER = re.compile(r"[+-]?[0-9]+\Z")   # what Rust's i64::from_str takes


def _concat_parts(parts, ranges):
    """(parts as lists of Column, kinds, part_rows, first, count) of a concat; the Python argument checks."""
    parts = [list(p) for p in parts]
    if not parts or not parts[0]:
        raise _capi.OxenError("concat needs at least one part of at least one column", _capi.OXH_ERR_INVALID)
    if len(parts) > _capi.OXH_CONCAT_MAX_PARTS:
        raise _capi.OxenError(f"concat takes at most OXH_CONCAT_MAX_PARTS = {_capi.OXH_CONCAT_MAX_PARTS} parts", _capi.OXH_ERR_INVALID)
    kinds = [int(c.kind) for c in parts[0]]
    for p, cols in enumerate(parts):
        if [int(c.kind) for c in cols] != kinds:
            raise _capi.OxenError(f"part {p} has other column kinds than part 0", _capi.OXH_ERR_INVALID)
        if any(c.nrows != cols[0].nrows for c in cols):
            raise _capi.OxenError(f"the columns of part {p} have one row count", _capi.OXH_ERR_INVALID)
    rows = [int(cols[0].nrows) for cols in parts]
    if ranges is None:
        return parts, kinds, rows, None, None
    ranges = [(int(f), int(n)) for f, n in ranges]
    if len(ranges) != len(parts):
        raise _capi.OxenError("one (first, count) per part", _capi.OXH_ERR_INVALID)
    for p, ((f, n), have) in enumerate(zip(ranges, rows)):
        if f < 0 or n < 0 or f + n > have:
            raise _capi.OxenError(f"part {p}: rows [{f}, {f + n}) of {have}", _capi.OXH_ERR_INVALID)
    return parts, kinds, rows, [f for f, _ in ranges], [n for _, n in ranges]


def _concat_head(parts, kinds, rows, first, count, ptr):
    """The ABI's arguments from nparts on to count."""
    flat = [c for cols in parts for c in cols]
    u64s = lambda v: None if v is None else (ctypes.c_uint64 * max(len(v), 1))(*v)   # noqa: E731
    return (len(parts), len(kinds), *_tables(flat, ptr), u64s(rows), u64s(first), u64s(count))


def _concat_result(parts, kinds, n, outs, view, i32, i64):
    result = []
    for c, (kind, (values, offsets, validity)) in enumerate(zip(kinds, outs)):
        src = parts[0][c].values
        if kind in _WIDTH and getattr(src, "dtype", None) is not None and view(src) == _WIDTH[kind]:
            values = values.view(src.dtype)
        offs = offsets.view(i32 if kind == OXH_COL_BYTES32 else i64) if kind in _BYTES else None
        result.append(Column(kind, n, values, offs, validity, 0, 0))
    return result


def concat(parts: Sequence, ranges=None, ctx: Optional[_capi.Context] = None) -> list:
    """oxh_concat_columns_host: rows [first, first + count) of each part, one part after the other. parts: a
    sequence of column sequences (`Column`s in host memory, the same kinds in the same order in every part; a
    part may be given twice); ranges: one (first, count) per part, None = whole parts. Returns the output
    `Column`s over fresh numpy buffers that start at bit / offset 0, validity always present, pad bits 0. Values
    are copied as they are, under null cells too (Arrow's own concat; the take zeroes them): sources in the
    take's canonical form give canonical output. The sizes-only call, the allocation, then the call that writes."""
    parts = [[c if isinstance(c, Column) else column(c) for c in p] for p in parts]
    parts, kinds, rows, first, count = _concat_parts(parts, ranges)
    n = sum(rows if count is None else count)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    ncols = len(kinds)
    value_bytes = (ctypes.c_uint64 * ncols)()
    written = ctypes.c_uint32(0)
    head = (_handle(ctx), *_concat_head(parts, kinds, rows, first, count, ptr))
    L = _capi.lib()
    _capi.check(L.oxh_concat_columns_host(*head, None, None, None, None, value_bytes, ctypes.byref(written)), "oxh_concat_columns_host")
    outs = [[np.zeros(size, dtype=np.uint8) for size in sizes] for sizes in _take_sizes(kinds, n, value_bytes)]
    capacity = (ctypes.c_uint64 * ncols)(*[o[0].size for o in outs])
    arrays = [_pointers([o[k].ctypes.data if o[k].size else None for o in outs]) for k in range(3)]
    _capi.check(L.oxh_concat_columns_host(*head, capacity, *arrays, value_bytes, ctypes.byref(written)), "oxh_concat_columns_host")
    if not written.value:
        raise _capi.OxenError("oxh_concat_columns_host: the columns changed between the two calls", _capi.OXH_ERR_INVALID)
    return _concat_result(parts, kinds, n, outs, lambda a: a.dtype.itemsize, np.int32, np.int64)


def concat_device(parts: Sequence, ranges=None, stream=None, ctx: Optional[_capi.Context] = None) -> list:
    """oxh_concat_columns_device: `concat` over `Column`s whose values / offsets / validity are torch tensors on
    the device. Nothing row-shaped crosses the link: the tables of pointers go up, two offsets per part and byte
    column come back. Returns `Column`s over fresh device tensors. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    parts, kinds, rows, first, count = _concat_parts(parts, ranges)
    tensors = [t for cols in parts for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    n = sum(rows if count is None else count)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    ncols = len(kinds)
    value_bytes = (ctypes.c_uint64 * ncols)()
    written = ctypes.c_uint32(0)
    head = (_handle(ctx), *_concat_head(parts, kinds, rows, first, count, ptr))
    L, st = _capi.lib(), _stream(stream)
    _capi.check(L.oxh_concat_columns_device(*head, None, None, None, None, value_bytes, ctypes.byref(written), st),
                "oxh_concat_columns_device")
    # not zero-filled: the call writes every byte (take_device says why)
    outs = [[torch.empty(size, dtype=torch.uint8, device=device) for size in sizes] for sizes in _take_sizes(kinds, n, value_bytes)]
    capacity = (ctypes.c_uint64 * ncols)(*[o[0].numel() for o in outs])
    arrays = [_pointers([ptr(o[k]) for o in outs]) for k in range(3)]
    _capi.check(L.oxh_concat_columns_device(*head, capacity, *arrays, value_bytes, ctypes.byref(written), st),
                "oxh_concat_columns_device")
    if not written.value:
        raise _capi.OxenError("oxh_concat_columns_device: the columns changed between the two calls", _capi.OXH_ERR_INVALID)
    return _concat_result(parts, kinds, n, outs, lambda t: t.element_size(), torch.int32, torch.int64)


def slice_range(nrows: int, offset: int, length: int) -> tuple:
    """(first, count) of polars' `slice(offset, length)` over nrows rows: a negative offset counts from the end;
    start = offset + nrows if offset < 0 else offset, stop = start + length, both clamped to [0, nrows]. Restated
    from polars' documented behaviour (the examples of `DataFrame.slice`); NOT pinned by a run of polars."""
    nrows, offset, length = int(nrows), int(offset), int(length)
    if nrows < 0 or length < 0:
        raise _capi.OxenError("nrows and length are not negative", _capi.OXH_ERR_INVALID)
    start = offset + nrows if offset < 0 else offset
    stop = start + length
    start, stop = min(max(start, 0), nrows), min(max(stop, 0), nrows)
    return start, stop - start


def parse_slice(text: str) -> tuple:
    """`--slice 0..10` as (start, end), with SliceRange's three refusals (opts/df_opts.rs:43-58, 93-108): not two
    whole numbers (i64) separated by the first '..'; a negative start; start >= end."""
    def invalid(reason):
        return _capi.OxenError(f"invalid data frame parameter slice = {text!r}: {reason}", _capi.OXH_ERR_INVALID)

    start, sep, end = str(text).partition("..")
    if not sep or not _SLICE_NUMBER.match(start) or not _SLICE_NUMBER.match(end):
        raise invalid("expected two whole numbers separated by '..', as '0..10'")
    start, end = int(start), int(end)
    if not -2 ** 63 <= start < 2 ** 63 or not -2 ** 63 <= end < 2 ** 63:
        raise invalid("expected two whole numbers separated by '..', as '0..10'")
    if start < 0:
        raise invalid("start must not be negative")
    if start >= end:
        raise invalid("start must be less than end")
    return start, end


def _frame_rows(frame: dict) -> int:
    cols = list(frame.values())
    if not cols:
        raise _capi.OxenError("a frame has at least one column", _capi.OXH_ERR_INVALID)
    if any(c.nrows != cols[0].nrows for c in cols):
        raise _capi.OxenError("the columns of a frame have one row count", _capi.OXH_ERR_INVALID)
    return int(cols[0].nrows)


def _slice_frame(frame, first_count, call, **kw) -> dict:
    return dict(zip(frame, call([list(frame.values())], [first_count], **kw)))


def slice_rows(frame: Mapping, offset: int, length: int, ctx: Optional[_capi.Context] = None) -> dict:
    """`oxen df --slice start..end` is slice_rows(frame, start, end - start) (core/df/tabular.rs:571-589): the
    rows `slice_range` names, through `concat`, as an ordered dict."""
    frame = _as_frame(frame)
    return _slice_frame(frame, slice_range(_frame_rows(frame), offset, length), concat, ctx=ctx)


def slice_rows_device(frame: Mapping, offset: int, length: int, stream=None, ctx: Optional[_capi.Context] = None) -> dict:
    """`slice_rows` over a frame of device `Column`s, through `concat_device`."""
    frame = dict(frame)
    return _slice_frame(frame, slice_range(_frame_rows(frame), offset, length), concat_device, stream=stream, ctx=ctx)


def head(frame: Mapping, n: int, ctx: Optional[_capi.Context] = None) -> dict:
    """`oxen df --head n`: slice(0, n)."""
    return slice_rows(frame, 0, n, ctx=ctx)


def head_device(frame: Mapping, n: int, stream=None, ctx: Optional[_capi.Context] = None) -> dict:
    return slice_rows_device(frame, 0, n, stream=stream, ctx=ctx)


def tail(frame: Mapping, n: int, ctx: Optional[_capi.Context] = None) -> dict:
    """`oxen df --tail n`: slice(-n, n)."""
    return slice_rows(frame, -int(n), n, ctx=ctx)


def tail_device(frame: Mapping, n: int, stream=None, ctx: Optional[_capi.Context] = None) -> dict:
    return slice_rows_device(frame, -int(n), n, stream=stream, ctx=ctx)


def page(frame: Mapping, page_size: int, page_num: int = 1, ctx: Optional[_capi.Context] = None) -> dict:
    """Page `page_num` of `page_size` rows of a data-frame view, the rows `page_rows` names (page_num 0 means 1,
    clipped to the frame)."""
    frame = _as_frame(frame)
    return _slice_frame(frame, page_rows(_frame_rows(frame), page_size, page_num), concat, ctx=ctx)


def page_device(frame: Mapping, page_size: int, page_num: int = 1, stream=None, ctx: Optional[_capi.Context] = None) -> dict:
    frame = dict(frame)
    return _slice_frame(frame, page_rows(_frame_rows(frame), page_size, page_num), concat_device, stream=stream, ctx=ctx)


def _vstack_frames(frames) -> list:
    frames = [dict(f) for f in frames]
    if not frames:
        raise _capi.OxenError("vstack needs at least one frame", _capi.OXH_ERR_INVALID)
    names = list(frames[0])
    for k, f in enumerate(frames[1:], 1):
        if list(f) != names:
            where = next((i for i, (a, b) in enumerate(zip(names, f)) if a != b), min(len(names), len(f)))
            have = list(f)[where] if where < len(f) else None
            want = names[where] if where < len(names) else None
            raise _capi.OxenError(f"vstack: frame {k} has column {have!r} where frame 0 has {want!r} (column {where}): the frames "
                                  "must have the same columns in the same order", _capi.OXH_ERR_INVALID)
        for name in names:
            if int(f[name].kind) != int(frames[0][name].kind):
                raise _capi.OxenError(f"vstack: column {name!r} of frame {k} has kind {int(f[name].kind)}, of frame 0 "
                                      f"{int(frames[0][name].kind)}", _capi.OXH_ERR_INVALID)
    return frames


def vstack(frames: Sequence[Mapping], ctx: Optional[_capi.Context] = None) -> dict:
    """`oxen df --vstack` (core/df/tabular.rs:449-463, polars' vertical concat): the frames' rows one frame after
    the other. The frames must have the same names in the same order and equal kinds; anything else raises
    OxenError(OXH_ERR_INVALID) naming the first mismatch. A `Column` does not tell Int32 from Float32: the dtype
    check beyond the kind stays with the caller's Arrow schema."""
    frames = _vstack_frames([_as_frame(f) for f in frames])
    return dict(zip(frames[0], concat([list(f.values()) for f in frames], ctx=ctx)))


def vstack_device(frames: Sequence[Mapping], stream=None, ctx: Optional[_capi.Context] = None) -> dict:
    """`vstack` over frames of device `Column`s, through `concat_device`."""
    frames = _vstack_frames(frames)
    return dict(zip(frames[0], concat_device([list(f.values()) for f in frames], stream=stream, ctx=ctx)))


# ---------------------------------------------------------------- CSV: record index and typed columns (oxh_csv_*)
CSV_TYPE_NAMES = {_capi.OXH_CSV_INT64: "Int64", _capi.OXH_CSV_FLOAT64: "Float64", _capi.OXH_CSV_BOOL: "Boolean",
                  _capi.OXH_CSV_STRING: "String", _capi.OXH_CSV_STRING64: "LargeString"}   # polars' dtype names
_CSV_TYPE_OF = {name: code for code, name in CSV_TYPE_NAMES.items()}


class CsvStats(NamedTuple):
    """stats8 of oxh_csv_open_*."""
    records: int
    rows: int
    ncols: int
    delimiters: int
    skipped_empty: int
    short_records: int
    long_records: int
    ended_in_quotes: int


class CsvColumnStats(NamedTuple):
    """stats4 of one selected column of oxh_csv_columns_*."""
    null_empty: int
    null_unparsable: int
    deferred: int
    value_bytes: int


def _csv_type(t) -> int:
    if isinstance(t, str):
        if t not in _CSV_TYPE_OF:
            raise _capi.OxenError(f"unknown CSV column type {t!r} (one of {sorted(_CSV_TYPE_OF)})", _capi.OXH_ERR_INVALID)
        return _CSV_TYPE_OF[t]
    return int(t)


def _csv_byte(ch, what, none=None) -> int:
    if ch is None and none is not None:
        return none
    raw = ch.encode("utf-8") if isinstance(ch, str) else bytes(ch)
    if len(raw) != 1:
        raise _capi.OxenError(f"the {what} is one byte, got {ch!r}", _capi.OXH_ERR_INVALID)
    return raw[0]


class CsvFile:
    """The record index of one CSV buffer (an oxh_csv_open_* handle): `stats`, `names`, `infer`, `measure`,
    `columns`. data: bytes / a uint8 numpy array (the host form, which owns a device copy), or with device=True a
    uint8 torch tensor on the device, which the object keeps alive. The rules are include/oxen_hash.h's "CSV": quotes
    by parity, records at '\\n' outside quotes, ragged records truncated or filled with nulls, unparsable text null.
    Dialect sniffing is the caller's: delimiter and quote_char are one byte each (quote_char None: no quoting)."""

    def __init__(self, data, delimiter=",", quote_char='"', has_header: bool = True, ctx: Optional[_capi.Context] = None,
                 device: bool = False, stream=None):
        self.device = device
        self.ctx = ctx
        self.stream = stream
        self.handle = None
        sep = _csv_byte(delimiter, "delimiter")
        quote = _csv_byte(quote_char, "quote", none=_capi.OXH_CSV_NO_QUOTE)
        flags = _capi.OXH_CSV_HAS_HEADER if has_header else 0
        out = ctypes.c_void_p()
        stats = np.zeros(8, dtype=np.uint64)
        if device:
            from .device import _require_cuda, _stream

            _require_cuda(data)
            if data.element_size() != 1 or not data.is_contiguous():
                raise _capi.OxenError("the CSV bytes are a contiguous uint8 tensor", _capi.OXH_ERR_INVALID)
            self.data = data
            _capi.check(_capi.lib().oxh_csv_open_device(_handle(ctx), data.data_ptr() if data.numel() else None, data.numel(), sep, quote,
                                                        flags, ctypes.byref(out), stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                        "oxh_csv_open_device")
        else:
            self.data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
            _capi.check(_capi.lib().oxh_csv_open_host(_handle(ctx), self.data.ctypes.data if self.data.size else None, self.data.size, sep,
                                                      quote, flags, ctypes.byref(out), stats.ctypes.data_as(_capi._u64p)),
                        "oxh_csv_open_host")
        self.handle = out
        self.stats = CsvStats(*(int(x) for x in stats))
        self.has_header = bool(has_header)
        self._names = None

    def close(self) -> None:
        if getattr(self, "handle", None):
            _capi.lib().oxh_csv_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def raw_names(self) -> list:
        """The header's names as bytes; without a header none."""
        if self._names is None:
            n = self.stats.ncols
            offsets, size = np.zeros(n + 1, dtype=np.uint64), ctypes.c_uint64(0)
            L = _capi.lib()
            _capi.check(L.oxh_csv_header(self.handle, None, 0, offsets.ctypes.data_as(_capi._u64p), ctypes.byref(size)), "oxh_csv_header")
            buf = np.zeros(max(size.value, 1), dtype=np.uint8)
            _capi.check(L.oxh_csv_header(self.handle, buf.ctypes.data, size.value, offsets.ctypes.data_as(_capi._u64p), ctypes.byref(size)),
                        "oxh_csv_header")
            raw = buf.tobytes()
            self._names = [raw[int(offsets[c]):int(offsets[c + 1])] for c in range(n)] if self.has_header else []
        return self._names

    @property
    def names(self) -> list:
        """The column names: the header's (invalid UTF-8 replaced, a repeated name as `name_duplicated_k`, polars'
        spelling), or column_1 .. without a header."""
        if not self.has_header:
            return [f"column_{c + 1}" for c in range(self.stats.ncols)]
        seen, out = {}, []
        for raw in self.raw_names:
            name = raw.decode("utf-8", errors="replace")
            k = seen.get(name, 0)
            seen[name] = k + 1
            out.append(name if k == 0 else f"{name}_duplicated_{k - 1}")
        return out

    def infer(self, rows: int = 10000) -> list:
        """oxh_csv_infer: one OXH_CSV_* per column from the first `rows` data rows."""
        types = (ctypes.c_uint32 * max(self.stats.ncols, 1))()
        _capi.check(_capi.lib().oxh_csv_infer(self.handle, int(rows), types), "oxh_csv_infer")
        return [int(types[c]) for c in range(self.stats.ncols)]

    def _selection(self, cols, types):
        cols, types = [int(c) for c in cols], [_csv_type(t) for t in types]
        if len(cols) != len(types):
            raise _capi.OxenError("one type per selected column", _capi.OXH_ERR_INVALID)
        n = max(len(cols), 1)
        return cols, types, (ctypes.c_uint32 * n)(*cols), (ctypes.c_uint32 * n)(*types)

    def _call(self, nsel, col_idx, type_words, capacity, values, offsets, validity):
        value_bytes, stats = np.zeros(max(nsel, 1), dtype=np.uint64), np.zeros(4 * max(nsel, 1), dtype=np.uint64)
        L = _capi.lib()
        args = (self.handle, nsel, col_idx, type_words, None if capacity is None else capacity.ctypes.data_as(_capi._u64p), values, offsets,
                validity, value_bytes.ctypes.data_as(_capi._u64p), stats.ctypes.data_as(_capi._u64p))
        if self.device:
            from .device import _stream

            _capi.check(L.oxh_csv_columns_device(*args, _stream(self.stream)), "oxh_csv_columns_device")
        else:
            _capi.check(L.oxh_csv_columns_host(*args), "oxh_csv_columns_host")
        return ([int(x) for x in value_bytes[:nsel]], [CsvColumnStats(*(int(x) for x in stats[4 * k:4 * k + 4])) for k in range(nsel)])

    def measure(self, cols, types):
        """(value_bytes, [CsvColumnStats]) of the selected columns without writing them."""
        cols, types, col_idx, type_words = self._selection(cols, types)
        return self._call(len(cols), col_idx, type_words, None, None, None, None)

    def columns(self, cols, types, with_stats: bool = False):
        """The selected columns (indices) as `Column`s of the given OXH_CSV_* types (or polars' dtype names): numpy
        arrays in the host form, torch tensors on the device in the device form. Validity is always there."""
        cols, types, col_idx, type_words = self._selection(cols, types)
        nsel, n = len(cols), self.stats.rows
        strings = [t in (_capi.OXH_CSV_STRING, _capi.OXH_CSV_STRING64) for t in types]
        sizes = [0] * nsel   # the bytes of the string columns, and only they are measured
        which = [k for k in range(nsel) if strings[k]]
        if which:
            for k, size in zip(which, self.measure([cols[k] for k in which], [types[k] for k in which])[0]):
                sizes[k] = size
        if self.device:
            import torch

            dev = self.data.device
            make = lambda count, dtype: torch.empty(count, dtype=dtype, device=dev)   # noqa: E731
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None      # noqa: E731
            i64, f64, u8, i32 = torch.int64, torch.float64, torch.uint8, torch.int32
        else:
            make = lambda count, dtype: np.zeros(count, dtype=dtype)                   # noqa: E731
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None        # noqa: E731
            i64, f64, u8, i32 = np.int64, np.float64, np.uint8, np.int32
        out = []
        capacity = np.zeros(max(nsel, 1), dtype=np.uint64)
        for k, t in enumerate(types):
            validity = make((n + 7) // 8, u8)
            if strings[k]:
                values, offsets = make(sizes[k], u8), make(n + 1, i64 if t == _capi.OXH_CSV_STRING64 else i32)
                if n == 0:
                    offsets[:] = 0
                capacity[k] = sizes[k]
                kind = OXH_COL_BYTES64 if t == _capi.OXH_CSV_STRING64 else OXH_COL_BYTES32
            elif t == _capi.OXH_CSV_BOOL:
                values, offsets, kind = make((n + 7) // 8, u8), None, OXH_COL_BOOL
                capacity[k] = (n + 7) // 8
            else:
                values, offsets, kind = make(n, i64 if t == _capi.OXH_CSV_INT64 else f64), None, OXH_COL_FIXED8
                capacity[k] = 8 * n
            out.append(Column(kind, n, values, offsets, validity))
        m = max(nsel, 1)
        tables = [(ctypes.c_void_p * m)(*[ptr(getattr(c, field)) for c in out]) for field in ("values", "offsets", "validity")]
        _, stats = self._call(nsel, col_idx, type_words, capacity, *tables)
        return (out, stats) if with_stats else out


def _csv_bytes(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        return path_or_bytes, None
    path = str(path_or_bytes)
    with open(path, "rb") as f:
        return f.read(), path


def _csv_delimiter(delimiter, path):
    # the reference sniffs the dialect (qsv_sniffer) and falls back to ','; sniffing stays with the caller, and a
    # .tsv file reads with tabs
    if delimiter is not None:
        return delimiter
    return "\t" if path is not None and path.lower().endswith(".tsv") else ","


def _csv_frame(f: CsvFile, schema, columns, infer_rows) -> dict:
    names = f.names
    if columns is None:
        picked = list(range(len(names)))
    else:
        picked = []
        for c in columns:
            if isinstance(c, str) and c not in names:
                raise _capi.OxenError(f"no column {c!r} in the CSV header {names}", _capi.OXH_ERR_INVALID)
            picked.append(names.index(c) if isinstance(c, str) else int(c))
    inferred = None
    types = []
    for c in picked:
        given = None if schema is None else (schema.get(names[c]) if isinstance(schema, Mapping) else schema[c])
        if given is None:
            inferred = inferred if inferred is not None else f.infer(infer_rows)
            given = inferred[c]
        types.append(_csv_type(given))
    return dict(zip([names[c] for c in picked], f.columns(picked, types)))


def read_csv(path_or_bytes, delimiter=None, quote_char='"', has_header: bool = True, schema=None, columns=None,
             infer_rows: int = 10000, ctx: Optional[_capi.Context] = None) -> dict:
    """`read_df_csv` (core/df/tabular.rs:39-71) on the device: a CSV file (a path) or its bytes to an ordered
    {name: Column} in host memory that every function of this module takes. delimiter: one byte; None reads a
    `.tsv` path with tabs and anything else with commas (the reference's sniffing stays with the caller).
    quote_char None: no quoting. schema: {name: type} or a sequence by column index, a type being an OXH_CSV_* code
    or polars' dtype name ("Int64", "Float64", "Boolean", "String", "LargeString"); columns without one are inferred
    from the first infer_rows rows (the reference's infer_schema_length). columns: the names or indices to read."""
    data, path = _csv_bytes(path_or_bytes)
    with CsvFile(data, _csv_delimiter(delimiter, path), quote_char, has_header, ctx=ctx) as f:
        return _csv_frame(f, schema, columns, infer_rows)


def read_csv_device(d_bytes, delimiter=",", quote_char='"', has_header: bool = True, schema=None, columns=None,
                    infer_rows: int = 10000, ctx: Optional[_capi.Context] = None, stream=None) -> dict:
    """`read_csv` over the file's bytes already on the device (a uint8 torch tensor, say after the add hashed
    them): device `Column`s that every `_device` function of this module accepts unchanged. Blocks."""
    with CsvFile(d_bytes, delimiter, quote_char, has_header, ctx=ctx, device=True, stream=stream) as f:
        return _csv_frame(f, schema, columns, infer_rows)


def csv_shape(path_or_bytes, delimiter=None, quote_char='"', has_header: bool = True, ctx: Optional[_capi.Context] = None) -> tuple:
    """(width, height) of the tabular metadata (repositories/metadata/tabular.rs:10-25): the columns and the data
    rows, by the index alone -- a newline inside a quoted field ends no record."""
    data, path = _csv_bytes(path_or_bytes)
    with CsvFile(data, _csv_delimiter(delimiter, path), quote_char, has_header, ctx=ctx) as f:
        return f.stats.ncols, f.stats.rows


def csv_schema(path_or_bytes, delimiter=None, quote_char='"', has_header: bool = True, infer_rows: int = 10000,
               ctx: Optional[_capi.Context] = None) -> list:
    """[(name, dtype name)] of the tabular metadata: the header's names and the inferred types."""
    data, path = _csv_bytes(path_or_bytes)
    with CsvFile(data, _csv_delimiter(delimiter, path), quote_char, has_header, ctx=ctx) as f:
        return list(zip(f.names, [CSV_TYPE_NAMES[t] for t in f.infer(infer_rows)]))


# ---------------------------------------------------------------- CSV text: typed columns to the file's bytes (oxh_write_csv_*)
class CsvWriteStats(NamedTuple):
    """stats4 of oxh_write_csv_*."""
    bytes: int
    quoted_cells: int
    deferred: int
    nulls: int


_WRITE_TYPE_OF_KIND = {OXH_COL_BOOL: _capi.OXH_CSV_BOOL, OXH_COL_BYTES32: _capi.OXH_CSV_STRING, OXH_COL_BYTES64: _capi.OXH_CSV_STRING64}
_WRITE_TYPE_OF_DTYPE = {"int64": _capi.OXH_CSV_INT64, "torch.int64": _capi.OXH_CSV_INT64,
                        "float64": _capi.OXH_CSV_FLOAT64, "torch.float64": _capi.OXH_CSV_FLOAT64}


def _write_types(names, cols, types) -> list:
    """One OXH_CSV_* per column: what `types` gives ({name: type} or a sequence by column), else what the Column's
    kind says, a FIXED8 column by its dtype."""
    out = []
    for k, (name, c) in enumerate(zip(names, cols)):
        given = None if types is None else (types.get(name) if isinstance(types, Mapping) else types[k])
        if given is not None:
            out.append(_csv_type(given))
        elif c.kind in _WRITE_TYPE_OF_KIND:
            out.append(_WRITE_TYPE_OF_KIND[c.kind])
        elif c.kind == OXH_COL_FIXED8 and str(getattr(c.values, "dtype", None)) in _WRITE_TYPE_OF_DTYPE:
            out.append(_WRITE_TYPE_OF_DTYPE[str(c.values.dtype)])
        else:
            raise _capi.OxenError(f"column {name!r} (kind {c.kind}, dtype {getattr(c.values, 'dtype', None)}) has no CSV text here: the "
                                  "writer takes Int64, Float64, Boolean and strings -- cast the column, or name its type in types=",
                                  _capi.OXH_ERR_INVALID)
    return out


def _write_head(frame: Mapping, delimiter, quote_char, include_header, types):
    """What both forms pass in front of the column tables and behind them."""
    names = list(frame.keys())
    cols = list(frame.values())
    if cols and any(c.nrows != cols[0].nrows for c in cols):
        raise _capi.OxenError("the columns of a frame have one row count", _capi.OXH_ERR_INVALID)
    n = max(len(cols), 1)
    type_words = (ctypes.c_uint32 * n)(*_write_types(names, cols, types))
    raw = [name.encode("utf-8") if isinstance(name, str) else bytes(name) for name in names]
    name_offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in raw], out=name_offsets[1:])
    name_bytes = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    tail = (_csv_byte(delimiter, "delimiter"), _csv_byte(quote_char, "quote", none=_capi.OXH_CSV_NO_QUOTE),
            _capi.OXH_CSV_HAS_HEADER if include_header else 0)
    return cols, type_words, name_bytes, name_offsets, tail


def _write_call(fn, what, ctx, cols, type_words, tables, name_bytes, name_offsets, tail, out, capacity, *stream):
    size, stats = ctypes.c_uint64(0), np.zeros(4, dtype=np.uint64)
    nrows = cols[0].nrows if cols else 0
    _capi.check(fn(_handle(ctx), nrows, len(cols), type_words, *tables, name_bytes.ctypes.data, name_offsets.ctypes.data_as(_capi._u64p),
                   *tail, out, capacity, ctypes.byref(size), stats.ctypes.data_as(_capi._u64p), *stream), what)
    return int(size.value), CsvWriteStats(*(int(x) for x in stats))


def write_csv(frame: Mapping, path=None, delimiter=",", quote_char='"', include_header: bool = True, types=None,
              ctx: Optional[_capi.Context] = None, with_stats: bool = False):
    """oxh_write_csv_host: the frame (an ordered {name: Column}, or what `column` takes, in host memory) as the bytes
    of a CSV file, by the rules of include/oxen_hash.h "CSV text" -- polars' CsvWriter as `write_df` configures it
    (core/df/tabular.rs:1492-1547). With a path the bytes are also written there, through `AtomicFile` as the
    reference does. types: {name: type} or a sequence by column for what the Column's kind does not say (a FIXED8
    column is typed by its int64 / float64 dtype). The mapping's key order is the column order; `str` keys go out as
    UTF-8."""
    frame = _as_frame(frame)
    cols, type_words, name_bytes, name_offsets, tail = _write_head(frame, delimiter, quote_char, include_header, types)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    tables = _tables(cols, ptr)
    fn = _capi.lib().oxh_write_csv_host
    need, _ = _write_call(fn, "oxh_write_csv_host", ctx, cols, type_words, tables, name_bytes, name_offsets, tail, None, 0)
    out = np.zeros(max(need, 1), dtype=np.uint8)
    need, stats = _write_call(fn, "oxh_write_csv_host", ctx, cols, type_words, tables, name_bytes, name_offsets, tail, out.ctypes.data, need)
    data = out[:need].tobytes()
    if path is not None:
        from .version_store import AtomicFile

        AtomicFile(path, ctx).write(data)
    return (data, stats) if with_stats else data


def write_csv_device(frame: Mapping, delimiter=",", quote_char='"', include_header: bool = True, types=None,
                     ctx: Optional[_capi.Context] = None, capacity: Optional[int] = None, stream=None, with_stats: bool = False):
    """oxh_write_csv_device: the same over device `Column`s (what `read_csv_device`, `take_device`, `concat_device`
    return); the file's bytes as a uint8 torch tensor on the device. It measures, allocates, then writes; a caller's
    `capacity` (bytes) skips the measure, and a capacity below the need is the library's error. Blocks."""
    import torch

    from .device import _require_cuda, _stream

    cols, type_words, name_bytes, name_offsets, tail = _write_head(frame, delimiter, quote_char, include_header, types)
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    tables = _tables(cols, ptr)
    fn = _capi.lib().oxh_write_csv_device
    head = (fn, "oxh_write_csv_device", ctx, cols, type_words, tables, name_bytes, name_offsets, tail)
    if capacity is None:
        capacity, _ = _write_call(*head, None, 0, _stream(stream))
    out = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=device)
    need, stats = _write_call(*head, out.data_ptr(), int(capacity), _stream(stream))
    return (out[:need], stats) if with_stats else out[:need]


# ---------------------------------------------------------------- JSON text: typed columns to the file's bytes (oxh_write_json_*)
class JsonWriteStats(NamedTuple):
    """stats4 of oxh_write_json_*."""
    bytes: int
    escaped_cells: int
    deferred: int
    nulls: int


def _json_head(frame: Mapping, types, flags):
    cols, type_words, name_bytes, name_offsets, _ = _write_head(frame, ",", '"', True, types)
    return cols, type_words, name_bytes, name_offsets, (flags,)


def _json_call(*args):
    need, stats = _write_call(*args)
    return need, JsonWriteStats(*stats)


def _write_json_host(frame, path, flags, types, ctx, with_stats):
    frame = _as_frame(frame)
    cols, type_words, name_bytes, name_offsets, tail = _json_head(frame, types, flags)
    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data if a.size else None

    tables = _tables(cols, ptr)
    head = (_capi.lib().oxh_write_json_host, "oxh_write_json_host", ctx, cols, type_words, tables, name_bytes, name_offsets, tail)
    need, _ = _json_call(*head, None, 0)
    out = np.zeros(max(need, 1), dtype=np.uint8)
    need, stats = _json_call(*head, out.ctypes.data, need)
    data = out[:need].tobytes()
    if path is not None:
        from .version_store import AtomicFile

        AtomicFile(path, ctx).write(data)
    return (data, stats) if with_stats else data


def _write_json_device(frame, flags, types, ctx, capacity, stream, with_stats):
    import torch

    from .device import _require_cuda, _stream

    cols, type_words, name_bytes, name_offsets, tail = _json_head(frame, types, flags)
    tensors = [t for c in cols for t in (c.values, c.offsets, c.validity) if t is not None]
    _require_cuda(*tensors)
    if any(not t.is_contiguous() for t in tensors):
        raise _capi.OxenError("column tensors must be contiguous", _capi.OXH_ERR_INVALID)
    device = tensors[0].device if tensors else "cuda"
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    tables = _tables(cols, ptr)
    head = (_capi.lib().oxh_write_json_device, "oxh_write_json_device", ctx, cols, type_words, tables, name_bytes, name_offsets, tail)
    if capacity is None:
        capacity, _ = _json_call(*head, None, 0, _stream(stream))
    out = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=device)
    need, stats = _json_call(*head, out.data_ptr(), int(capacity), _stream(stream))
    return (out[:need], stats) if with_stats else out[:need]


def write_jsonl(frame: Mapping, path=None, types=None, ctx: Optional[_capi.Context] = None, with_stats: bool = False):
    """oxh_write_json_host with OXH_JSON_LINES: the frame (an ordered {name: Column}, or what `column` takes, in host
    memory) as the bytes of a JSON Lines file, by the rules of include/oxen_hash.h "JSON text" -- polars' JsonWriter
    with JsonFormat::JsonLines, `write_df`'s jsonl / ndjson arm (core/df/tabular.rs:1469-1490). path, types and the
    key order are `write_csv`'s."""
    return _write_json_host(frame, path, _capi.OXH_JSON_LINES, types, ctx, with_stats)


def write_json(frame: Mapping, path=None, types=None, ctx: Optional[_capi.Context] = None, with_stats: bool = False):
    """oxh_write_json_host with OXH_JSON_ARRAY: one array of the rows' objects -- JsonFormat::Json, `write_df`'s json
    arm and the text of a data-frame view (view/json_data_frame_view.rs:268-285)."""
    return _write_json_host(frame, path, _capi.OXH_JSON_ARRAY, types, ctx, with_stats)


def write_jsonl_device(frame: Mapping, types=None, ctx: Optional[_capi.Context] = None, capacity: Optional[int] = None, stream=None,
                       with_stats: bool = False):
    """oxh_write_json_device with OXH_JSON_LINES over device `Column`s; the file's bytes as a uint8 torch tensor on the
    device. It measures, allocates, then writes; a caller's `capacity` (bytes) skips the measure, and a capacity
    below the need is the library's error. Blocks."""
    return _write_json_device(frame, _capi.OXH_JSON_LINES, types, ctx, capacity, stream, with_stats)


def write_json_device(frame: Mapping, types=None, ctx: Optional[_capi.Context] = None, capacity: Optional[int] = None, stream=None,
                      with_stats: bool = False):
    """oxh_write_json_device with OXH_JSON_ARRAY: what `json_from_df` makes of a page built on the device."""
    return _write_json_device(frame, _capi.OXH_JSON_ARRAY, types, ctx, capacity, stream, with_stats)


def write_df(frame: Mapping, path, ctx: Optional[_capi.Context] = None) -> bytes:
    """`write_df` (core/df/tabular.rs:1529-1547) for the text formats this module writes: `.csv` with ',', `.tsv` with
    '\\t', `.jsonl` / `.ndjson` as JSON Lines and `.json` as one array. Any other extension raises the reference's
    "Unknown file type" error."""
    import os

    path = str(path)
    ext = os.path.splitext(path)[1][1:] or None
    if ext == "csv":
        return write_csv(frame, path, ",", ctx=ctx)
    if ext == "tsv":
        return write_csv(frame, path, "\t", ctx=ctx)
    if ext in ("jsonl", "ndjson"):
        return write_jsonl(frame, path, ctx=ctx)
    if ext == "json":
        return write_json(frame, path, ctx=ctx)
    shown = "None" if ext is None else f'Some("{ext}")'
    raise _capi.OxenError(f'Unknown file type write_df "{path}" {shown}', _capi.OXH_ERR_INVALID)


# ---------------------------------------------------------------- JSON Lines: record index and typed columns (oxh_jsonl_*)
_READ_ERROR = "Could not read tabular data from path"   # the reference's OxenError::basic_str of a failed read


class JsonlStats(NamedTuple):
    """stats8 of oxh_jsonl_open_*."""
    records: int
    rows: int
    ncols: int
    malformed: int
    skipped_blank: int
    non_canonical: int
    ignored_fields: int
    nested_values: int


class JsonlFile:
    """The record index of one JSON Lines buffer (an oxh_jsonl_open_* handle), the twin of `CsvFile`: `stats`,
    `names`, `infer`, `measure`, `columns`. data: bytes / a uint8 numpy array (the host form, which owns a device
    copy), or with device=True a uint8 torch tensor on the device, which the object keeps alive. The rules are
    include/oxen_hash.h's "JSON Lines": a record per line, the names in order of first appearance over the first
    infer_rows rows, a malformed record or an unparsable cell null."""

    def __init__(self, data, infer_rows: int = 10000, ctx: Optional[_capi.Context] = None, device: bool = False, stream=None):
        self.device = device
        self.ctx = ctx
        self.stream = stream
        self.handle = None
        window = (1 << 64) - 1 if infer_rows is None else int(infer_rows)
        out = ctypes.c_void_p()
        stats = np.zeros(8, dtype=np.uint64)
        if device:
            from .device import _require_cuda, _stream

            _require_cuda(data)
            if data.element_size() != 1 or not data.is_contiguous():
                raise _capi.OxenError("the JSON Lines bytes are a contiguous uint8 tensor", _capi.OXH_ERR_INVALID)
            self.data = data
            _capi.check(_capi.lib().oxh_jsonl_open_device(_handle(ctx), data.data_ptr() if data.numel() else None, data.numel(), window, 0,
                                                          ctypes.byref(out), stats.ctypes.data_as(_capi._u64p), _stream(stream)),
                        "oxh_jsonl_open_device")
        else:
            self.data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
            _capi.check(_capi.lib().oxh_jsonl_open_host(_handle(ctx), self.data.ctypes.data if self.data.size else None, self.data.size, window,
                                                        0, ctypes.byref(out), stats.ctypes.data_as(_capi._u64p)),
                        "oxh_jsonl_open_host")
        self.handle = out
        self.stats = JsonlStats(*(int(x) for x in stats))
        self._names = None

    def close(self) -> None:
        if getattr(self, "handle", None):
            _capi.lib().oxh_jsonl_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def raw_names(self) -> list:
        """The unescaped names as bytes."""
        if self._names is None:
            n = self.stats.ncols
            offsets, size = np.zeros(n + 1, dtype=np.uint64), ctypes.c_uint64(0)
            L = _capi.lib()
            _capi.check(L.oxh_jsonl_names(self.handle, None, 0, offsets.ctypes.data_as(_capi._u64p), ctypes.byref(size)), "oxh_jsonl_names")
            buf = np.zeros(max(size.value, 1), dtype=np.uint8)
            _capi.check(L.oxh_jsonl_names(self.handle, buf.ctypes.data, size.value, offsets.ctypes.data_as(_capi._u64p), ctypes.byref(size)),
                        "oxh_jsonl_names")
            raw = buf.tobytes()
            self._names = [raw[int(offsets[c]):int(offsets[c + 1])] for c in range(n)]
        return self._names

    @property
    def names(self) -> list:
        """The column names (invalid UTF-8 replaced; the names of one file are distinct as bytes)."""
        return [raw.decode("utf-8", errors="replace") for raw in self.raw_names]

    def infer(self) -> list:
        """oxh_jsonl_infer: one OXH_CSV_* per column from the window given at open."""
        types = (ctypes.c_uint32 * max(self.stats.ncols, 1))()
        _capi.check(_capi.lib().oxh_jsonl_infer(self.handle, types), "oxh_jsonl_infer")
        return [int(types[c]) for c in range(self.stats.ncols)]

    _selection = CsvFile._selection

    def _call(self, nsel, col_idx, type_words, capacity, values, offsets, validity):
        value_bytes, stats = np.zeros(max(nsel, 1), dtype=np.uint64), np.zeros(4 * max(nsel, 1), dtype=np.uint64)
        L = _capi.lib()
        args = (self.handle, nsel, col_idx, type_words, None if capacity is None else capacity.ctypes.data_as(_capi._u64p), values, offsets,
                validity, value_bytes.ctypes.data_as(_capi._u64p), stats.ctypes.data_as(_capi._u64p))
        if self.device:
            from .device import _stream

            _capi.check(L.oxh_jsonl_columns_device(*args, _stream(self.stream)), "oxh_jsonl_columns_device")
        else:
            _capi.check(L.oxh_jsonl_columns_host(*args), "oxh_jsonl_columns_host")
        return ([int(x) for x in value_bytes[:nsel]], [CsvColumnStats(*(int(x) for x in stats[4 * k:4 * k + 4])) for k in range(nsel)])

    measure = CsvFile.measure
    columns = CsvFile.columns


def _jsonl_frame(f: JsonlFile, schema, columns, ignore_errors: bool) -> dict:
    names = f.names
    if columns is None:
        picked = list(range(len(names)))
    else:
        picked = []
        for c in columns:
            if isinstance(c, str) and c not in names:
                raise _capi.OxenError(f"no column {c!r} among the JSON Lines names {names}", _capi.OXH_ERR_INVALID)
            picked.append(names.index(c) if isinstance(c, str) else int(c))
    inferred = None
    types = []
    for c in picked:
        given = None if schema is None else (schema.get(names[c]) if isinstance(schema, Mapping) else schema[c])
        if given is None:
            inferred = inferred if inferred is not None else f.infer()
            given = inferred[c]
        types.append(_csv_type(given))
    cols, stats = f.columns(picked, types, with_stats=True)
    if not ignore_errors and (f.stats.malformed or any(s.null_unparsable for s in stats)):
        raise _capi.OxenError(_READ_ERROR, _capi.OXH_ERR_INVALID)
    return dict(zip([names[c] for c in picked], cols))


def read_jsonl(path_or_bytes, schema=None, columns=None, infer_rows: int = 10000, ignore_errors: bool = False,
               ctx: Optional[_capi.Context] = None) -> dict:
    """`read_df_jsonl` (core/df/tabular.rs:73-82) on the device: a JSON Lines file (a path) or its bytes to the
    ordered {name: Column} in host memory that every function of this module takes. schema and columns as
    `read_csv`'s; columns without a type are inferred from the first infer_rows rows, which are also the rows whose
    keys name the columns. A malformed record, or an unparsable cell in a selected column, raises the reference's
    "Could not read tabular data from path"; with ignore_errors=True those cells are null."""
    data, _ = _csv_bytes(path_or_bytes)
    with JsonlFile(data, infer_rows, ctx=ctx) as f:
        return _jsonl_frame(f, schema, columns, ignore_errors)


def read_jsonl_device(d_bytes, schema=None, columns=None, infer_rows: int = 10000, ignore_errors: bool = False,
                      ctx: Optional[_capi.Context] = None, stream=None) -> dict:
    """`read_jsonl` over the file's bytes already on the device (a uint8 torch tensor): device `Column`s that every
    `_device` function of this module accepts unchanged. Blocks."""
    with JsonlFile(d_bytes, infer_rows, ctx=ctx, device=True, stream=stream) as f:
        return _jsonl_frame(f, schema, columns, ignore_errors)


def jsonl_shape(path_or_bytes, infer_rows: int = 10000, ctx: Optional[_capi.Context] = None) -> tuple:
    """(width, height) of the tabular metadata: the names and the records, by the index alone."""
    data, _ = _csv_bytes(path_or_bytes)
    with JsonlFile(data, infer_rows, ctx=ctx) as f:
        return f.stats.ncols, f.stats.rows


def jsonl_schema(path_or_bytes, infer_rows: int = 10000, ctx: Optional[_capi.Context] = None) -> list:
    """[(name, dtype name)] of the tabular metadata: the names and the inferred types."""
    data, _ = _csv_bytes(path_or_bytes)
    with JsonlFile(data, infer_rows, ctx=ctx) as f:
        return list(zip(f.names, [CSV_TYPE_NAMES[t] for t in f.infer()]))


def read_df(path, ctx: Optional[_capi.Context] = None) -> dict:
    """`read_df` (core/df/tabular.rs:1032-1048 and the arms of :1077-1103) for the text formats this module reads, the
    twin of `write_df`: `.csv`, `.data` and `.tsv` through `read_csv`, `.jsonl` and `.ndjson` through `read_jsonl`.
    `.json`, `.parquet` and `.arrow` are forms this module does not read. Any other extension raises the text of the
    `_` arm (:1097-1101); a path without an extension that of the earlier branch (:1044-1045), which prints the
    Option as `None`."""
    import os

    path = str(path)
    ext = os.path.splitext(path)[1][1:]
    if ext in ("csv", "data", "tsv"):
        return read_csv(path, ctx=ctx)
    if ext in ("jsonl", "ndjson"):
        return read_jsonl(path, ctx=ctx)
    if ext in ("json", "parquet", "arrow"):
        raise _capi.OxenError(f'reading the "{ext}" form is not built: {path}', _capi.OXH_ERR_INVALID)
    # Rust's {path:?} quotes the path; a path without an extension prints its Option as None
    raise _capi.OxenError(f'Could not load data frame with path: "{path}" and extension: {ext or "None"}', _capi.OXH_ERR_INVALID)
