"""Block-level dedup chunkers on the GPU.

Fixed-size chunkers (experiments/block-level-dedup/src/chunker/fixedsize.rs, `FixedSizeChunker`, and
fixedsize_multithreaded.rs, `FixedSizeMultiChunker`): a file is cut into chunk_size pieces (the last
one shorter), each piece is named by the decimal xxh3_128 of its bytes and written to output_dir
unless a chunk of that name exists; metadata.bin lists the names (bincode). Here the file is read in
segments of whole chunks, each segment goes to the device once and `oxh_chunk_digests_device` hashes
all its chunks in one launch; the chunk files are written by `concurrency` host threads.

FastCDC (fastcdchunker.rs, `FastCDChunker`): the file is
chunked with FastCDC v2020 (min 4096, avg = chunk_size, max = 2 * chunk_size, :55-57, :83-88) and
every chunk is written to `output_dir/<decimal xxh3_128 of the chunk>` (:96-107); the chunk names go
to `metadata.bin` as bincode 1.x of `ChunkMetadata {original_file_name: String, original_file_size:
u64, chunks: Vec<String>}` (:11-16, :110-121). Boundaries and digests both come from the GPU
(`oxh_fastcdc_device`: FastCDC candidate scan + speculative walks + K1 over the chunk table).
"""
from __future__ import annotations

import ctypes
import os
import struct
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _capi
from .device import fastcdc_device, to_numpy_u64

METADATA_FILE_NAME = "metadata.bin"  # fastcdchunker.rs:18
MIN_CHUNK_SIZE = 4096                # fastcdchunker.rs:55


def chunk_name(lo: int, hi: int) -> str:
    """u128::to_string() of the chunk digest (fastcdchunker.rs:98)."""
    return str((int(hi) << 64) | int(lo))


def _bincode_string(s: str) -> bytes:
    b = s.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def encode_metadata(original_file_name: str, original_file_size: int, chunks: list[str]) -> bytes:
    """bincode 1.x default (fixint, little-endian, u64 lengths) of ChunkMetadata."""
    out = [_bincode_string(original_file_name), struct.pack("<Q", original_file_size), struct.pack("<Q", len(chunks))]
    out += [_bincode_string(c) for c in chunks]
    return b"".join(out)


class _Bincode:
    """A reader over bincode 1.x default encoding (fixint, little-endian, u64 lengths)."""

    def __init__(self, buf: bytes):
        self.buf, self.pos = buf, 0

    def take(self, n: int) -> bytes:
        if self.pos + n > len(self.buf):
            raise _capi.OxenError("Bincode error: unexpected end of metadata", _capi.OXH_ERR_IO)
        v = self.buf[self.pos:self.pos + n]
        self.pos += n
        return v

    def u64(self) -> int:
        return struct.unpack("<Q", self.take(8))[0]

    def u8(self) -> int:
        return self.take(1)[0]

    def string(self) -> str:
        return self.take(self.u64()).decode("utf-8")

    def strings(self) -> list[str]:
        return [self.string() for _ in range(self.u64())]


def decode_metadata(buf: bytes) -> tuple[str, int, list[str]]:
    r = _Bincode(buf)
    name = r.string()
    size = r.u64()
    return name, size, r.strings()


def _strings(items: list[str]) -> bytes:
    return struct.pack("<Q", len(items)) + b"".join(_bincode_string(c) for c in items)


def encode_fixed_metadata(original_file_name: str, original_file_size: int, chunk_size: int, chunks: list[str]) -> bytes:
    """fixedsize_multithreaded.rs:14-20 ChunkMetadata {original_file_name, original_file_size: u64,
    chunk_size: usize, chunks: Vec<String>} in bincode 1.x."""
    return (_bincode_string(original_file_name) + struct.pack("<QQ", original_file_size, chunk_size) + _strings(chunks))


def decode_fixed_metadata(buf: bytes) -> tuple[str, int, int, list[str]]:
    r = _Bincode(buf)
    name = r.string()
    size, chunk = r.u64(), r.u64()
    return name, size, chunk, r.strings()


def encode_archive_metadata(chunk_size: int, entries: list[dict]) -> bytes:
    """fixedsize.rs:22-35 ArchiveMetadata {chunk_size: usize, entries: Vec<ArchiveEntry {path: PathBuf,
    is_dir: bool, chunks: Option<Vec<String>>, size: Option<u64>}>} in bincode 1.x (Option = u8 tag)."""
    out = [struct.pack("<QQ", chunk_size, len(entries))]
    for e in entries:
        out.append(_bincode_string(e["path"]))
        out.append(b"\x01" if e["is_dir"] else b"\x00")
        out.append(b"\x00" if e["chunks"] is None else b"\x01" + _strings(e["chunks"]))
        out.append(b"\x00" if e["size"] is None else b"\x01" + struct.pack("<Q", e["size"]))
    return b"".join(out)


def decode_archive_metadata(buf: bytes) -> tuple[int, list[dict]]:
    r = _Bincode(buf)
    chunk = r.u64()
    entries = []
    for _ in range(r.u64()):
        path = r.string()
        is_dir = r.u8() != 0
        chunks = r.strings() if r.u8() else None
        size = r.u64() if r.u8() else None
        entries.append({"path": path, "is_dir": is_dir, "chunks": chunks, "size": size})
    return chunk, entries


class FastCdcTable:
    """A chunk table in host memory: chunk k = bytes [offsets[k], offsets[k] + lens[k]) of its file,
    digests[k] = (lo, hi) of its XXH3-128 (None when not asked for); file i's chunks are rows
    first[i] .. first[i+1]-1. sizes / status / os_error per file (oxh_fastcdc_files)."""

    def __init__(self, offsets, lens, digests, first, sizes=None, status=None, os_error=None):
        self.offsets, self.lens, self.digests, self.first = offsets, lens, digests, first
        self.sizes, self.status, self.os_error = sizes, status, os_error

    def file(self, i: int):
        a, b = int(self.first[i]), int(self.first[i + 1])
        return self.offsets[a:b], self.lens[a:b], (self.digests[a:b] if self.digests is not None else None)


def _need_from_error(e: _capi.OxenError) -> Optional[int]:
    import re

    m = re.search(r"need (\d+) entries", str(e))
    return int(m.group(1)) if m and e.code == _capi.OXH_ERR_INVALID else None


def _ctx_array(ctxs):
    arr = (ctypes.c_void_p * len(ctxs))(*[c.handle.value if isinstance(c.handle, ctypes.c_void_p) else c.handle
                                          for c in ctxs])
    return arr


def fastcdc_files(paths, min_size: int, avg_size: int, max_size: int, level: int = 1, digests: bool = True,
                  ctx: Optional[_capi.Context] = None, ctxs=None) -> FastCdcTable:
    """oxh_fastcdc_files: FastCDC v2020 boundaries and XXH3-128 chunk digests of files on disk, read by
    the library (fastcdchunker.rs:75-98: fs::read, v2020 chunking, xxh3_128 per chunk), results in
    host memory. A file that cannot be opened / read has no chunks and its status / errno set.
    ctxs (several contexts, e.g. one per device): oxh_fastcdc_files_multi, the files shared out."""
    from .hasher import _PathTable, default_context

    ctx = ctx or (None if ctxs else default_context())
    n = len(paths)
    sizes_hint = np.zeros(n, dtype=np.uint64)
    for i, p in enumerate(paths):
        try:
            sizes_hint[i] = os.stat(p).st_size
        except OSError:
            pass
    L = _capi.lib()
    cap = max(1, int(L.oxh_fastcdc_max_chunks(sizes_hint.ctypes.data_as(_capi._u64p), n, max(1, int(min_size)))))
    table = _PathTable(paths) if n else None
    for _ in range(3):  # a file that grew since the stat above needs a larger table: retry with the count
        off = np.zeros(cap, dtype=np.uint64)
        ln = np.zeros(cap, dtype=np.uint64)
        dig = np.zeros((cap, 2), dtype=np.uint64) if digests else None
        first = np.zeros(n + 1, dtype=np.uint64)
        sizes = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        oserr = np.zeros(n, dtype=np.int32)
        tail = (int(min_size), int(avg_size), int(max_size), int(level), off.ctypes.data_as(_capi._u64p),
                ln.ctypes.data_as(_capi._u64p), dig.ctypes.data_as(_capi._u64p) if dig is not None else None, cap,
                first.ctypes.data_as(_capi._u64p), sizes.ctypes.data_as(_capi._u64p), status.ctypes.data_as(_capi._i32p),
                oserr.ctypes.data_as(_capi._i32p))
        if ctxs:
            rc = L.oxh_fastcdc_files_multi(_ctx_array(ctxs), len(ctxs), table.arg if table else None, n, *tail)
        else:
            rc = L.oxh_fastcdc_files(ctx.handle, table.arg if table else None, n, *tail)
        try:
            _capi.check(rc, "oxh_fastcdc_files")
        except _capi.OxenError as e:
            need = _need_from_error(e)
            if need is None:
                raise
            cap = need
            continue
        total = int(first[n])
        return FastCdcTable(off[:total], ln[:total], dig[:total] if dig is not None else None, first, sizes, status, oserr)
    raise _capi.OxenError("oxh_fastcdc_files: the files keep growing", _capi.OXH_ERR_INVALID)


def fastcdc_host(buffers, min_size: int, avg_size: int, max_size: int, level: int = 1, digests: bool = True,
                 ctx: Optional[_capi.Context] = None, ctxs=None) -> FastCdcTable:
    """oxh_fastcdc_host: the same over host buffers (bytes / numpy uint8 arrays); ctxs: over several
    contexts (oxh_fastcdc_host_multi)."""
    from .hasher import default_context

    ctx = ctx or (None if ctxs else default_context())
    arrs = [np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else np.ascontiguousarray(b, dtype=np.uint8)
            for b in buffers]
    n = len(arrs)
    lens_in = np.array([a.size for a in arrs], dtype=np.uint64)
    ptrs = (ctypes.c_char_p * max(n, 1))(*[ctypes.cast(a.ctypes.data, ctypes.c_char_p) if a.size else None for a in arrs])
    L = _capi.lib()
    cap = max(1, int(L.oxh_fastcdc_max_chunks(lens_in.ctypes.data_as(_capi._u64p), n, max(1, int(min_size)))))
    off = np.zeros(cap, dtype=np.uint64)
    ln = np.zeros(cap, dtype=np.uint64)
    dig = np.zeros((cap, 2), dtype=np.uint64) if digests else None
    first = np.zeros(n + 1, dtype=np.uint64)
    tail = (lens_in.ctypes.data_as(_capi._u64p), n, int(min_size), int(avg_size), int(max_size), int(level),
            off.ctypes.data_as(_capi._u64p), ln.ctypes.data_as(_capi._u64p),
            dig.ctypes.data_as(_capi._u64p) if dig is not None else None, cap, first.ctypes.data_as(_capi._u64p))
    if ctxs:
        _capi.check(L.oxh_fastcdc_host_multi(_ctx_array(ctxs), len(ctxs), ptrs, *tail), "oxh_fastcdc_host_multi")
    else:
        _capi.check(L.oxh_fastcdc_host(ctx.handle, ptrs, *tail), "oxh_fastcdc_host")
    total = int(first[n])
    return FastCdcTable(off[:total], ln[:total], dig[:total] if dig is not None else None, first)


class FixedChunkTable:
    """Fixed-size chunk digests in host memory (oxh_chunk_digests_files / _host): digests[k] = (lo, hi)
    of chunk k; file i's chunks are rows first[i] .. first[i+1]-1, chunk j of a file being its bytes
    [j*chunk, min((j+1)*chunk, size)). sizes per file; status / os_error per file (files only).
    chunk_size is what the table was cut at (the chunk lengths follow from it and sizes)."""

    def __init__(self, digests, first, sizes=None, status=None, os_error=None, chunk_size=None):
        self.digests, self.first, self.sizes, self.status, self.os_error = digests, first, sizes, status, os_error
        self.chunk_size = chunk_size

    def file(self, i: int):
        return self.digests[int(self.first[i]):int(self.first[i + 1])]


def _fixed_count(sizes, chunk: int) -> int:
    return int(sum((int(x) + chunk - 1) // chunk for x in sizes))


# Measured rates behind INTEGRATION.md §2 "When NOT to call the host chunk entries" (DESIGN §5,
# profiles/r05/r05j_fixed_e2e_*, r05as_h2d_probe.json): host-resident bytes cross one PCIe link per GPU
# first (~49 GiB/s each, the host entries at 92-93 % of the link), the reference's CPU loops hash at
# these rates per core (16 threads: fixed-size 67.7 GiB/s, FastCDC 34.9-40.3 GiB/s).
LINK_GIBS = 49.0
CPU_GIBS_PER_CORE = {"fixed": 4.2, "fastcdc": 2.4}


def host_entry_pays_off(host_cores: int, links: int, fastcdc: bool) -> bool:
    """Whether chunk_digests_files / fastcdc_files (and _multi) beat the reference's own CPU loop for
    host-resident files on this node: links x LINK_GIBS against host_cores x the per-core rate. A
    routing rule for the caller (bytes already in HBM take the device entries regardless); the library
    itself has no CPU hashing path."""
    cpu = host_cores * CPU_GIBS_PER_CORE["fastcdc" if fastcdc else "fixed"]
    return links * LINK_GIBS > cpu


def chunk_digests_files(paths, chunk_size: int, ctx: Optional[_capi.Context] = None, ctxs=None) -> FixedChunkTable:
    """oxh_chunk_digests_files: XXH3-128 of every fixed-size chunk of files on disk, read by the library
    (fixedsize_multithreaded.rs:78-110), digests in host memory; per-file errors as fastcdc_files.
    ctxs: oxh_chunk_digests_files_multi over several contexts."""
    from .hasher import _PathTable, default_context

    if chunk_size <= 0:
        raise _capi.OxenError("Chunk size cannot be zero", _capi.OXH_ERR_INVALID)
    ctx = ctx or (None if ctxs else default_context())
    n = len(paths)
    hint = []
    for p in paths:
        try:
            hint.append(os.stat(p).st_size)
        except OSError:
            hint.append(0)
    cap = max(1, _fixed_count(hint, chunk_size))
    table = _PathTable(paths) if n else None
    L = _capi.lib()
    for _ in range(3):  # a file that grew since the stat above: retry with the count the call reports
        dig = np.zeros((cap, 2), dtype=np.uint64)
        first = np.zeros(n + 1, dtype=np.uint64)
        sizes = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        oserr = np.zeros(n, dtype=np.int32)
        tail = (int(chunk_size), dig.ctypes.data_as(_capi._u64p), cap, first.ctypes.data_as(_capi._u64p),
                sizes.ctypes.data_as(_capi._u64p), status.ctypes.data_as(_capi._i32p), oserr.ctypes.data_as(_capi._i32p))
        if ctxs:
            rc = L.oxh_chunk_digests_files_multi(_ctx_array(ctxs), len(ctxs), table.arg if table else None, n, *tail)
        else:
            rc = L.oxh_chunk_digests_files(ctx.handle, table.arg if table else None, n, *tail)
        try:
            _capi.check(rc, "oxh_chunk_digests_files")
        except _capi.OxenError as e:
            need = _need_from_error(e)
            if need is None:
                raise
            cap = need
            continue
        return FixedChunkTable(dig[:int(first[n])], first, sizes, status, oserr, chunk_size=int(chunk_size))
    raise _capi.OxenError("oxh_chunk_digests_files: the files keep growing", _capi.OXH_ERR_INVALID)


def chunk_digests_host(buffers, chunk_size: int, ctx: Optional[_capi.Context] = None, ctxs=None) -> FixedChunkTable:
    """oxh_chunk_digests_host: the same over host buffers (bytes / numpy uint8 arrays); ctxs: over
    several contexts (oxh_chunk_digests_host_multi)."""
    from .hasher import default_context

    if chunk_size <= 0:
        raise _capi.OxenError("Chunk size cannot be zero", _capi.OXH_ERR_INVALID)
    ctx = ctx or (None if ctxs else default_context())
    arrs = [np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else np.ascontiguousarray(b, dtype=np.uint8)
            for b in buffers]
    n = len(arrs)
    lens_in = np.array([a.size for a in arrs], dtype=np.uint64)
    ptrs = (ctypes.c_char_p * max(n, 1))(*[ctypes.cast(a.ctypes.data, ctypes.c_char_p) if a.size else None for a in arrs])
    cap = max(1, _fixed_count(lens_in, chunk_size))
    dig = np.zeros((cap, 2), dtype=np.uint64)
    first = np.zeros(n + 1, dtype=np.uint64)
    tail = (lens_in.ctypes.data_as(_capi._u64p), n, int(chunk_size), dig.ctypes.data_as(_capi._u64p), cap,
            first.ctypes.data_as(_capi._u64p))
    if ctxs:
        _capi.check(_capi.lib().oxh_chunk_digests_host_multi(_ctx_array(ctxs), len(ctxs), ptrs, *tail),
                    "oxh_chunk_digests_host_multi")
    else:
        _capi.check(_capi.lib().oxh_chunk_digests_host(ctx.handle, ptrs, *tail), "oxh_chunk_digests_host")
    return FixedChunkTable(dig[:int(first[n])], first, sizes=lens_in, chunk_size=int(chunk_size))


ABSENT = (1 << 64) - 1  # DedupIndex.query: no row carries this digest


class DedupStats(NamedTuple):
    """One insert: rows that brought a digest the index had not seen (and their bytes), rows that
    repeated one (and theirs)."""
    new_rows: int
    new_bytes: int
    dup_rows: int
    dup_bytes: int


class DedupCounts(NamedTuple):
    """An index's lifetime: rows inserted, distinct digests among them, their bytes, distinct bytes."""
    rows: int
    distinct: int
    bytes: int
    distinct_bytes: int


def _digest_rows(digests) -> np.ndarray:
    a = np.ascontiguousarray(digests, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 2:
        if a.size == 0:
            return a.reshape(0, 2)
        raise _capi.OxenError("digests must be an (n, 2) uint64 array of (lo, hi) rows", _capi.OXH_ERR_INVALID)
    return a


class DedupIndex:
    """oxh_dedup_index_*: a hash table in device memory keyed by 128-bit chunk digests, persistent
    across calls. Every inserted row has an ordinal (rows inserted before its call + its position in
    the call); `insert` returns, per row, the smallest ordinal that carries the same digest, so a row is
    a first occurrence exactly when that is its own ordinal. Replaces the per-chunk
    `chunk_path.exists()` of fixedsize.rs:78-89 and the write-everything of fastcdchunker.rs:95-108.
    The index uses its context's device and streams: close it before the context."""

    def __init__(self, ctx: Optional[_capi.Context] = None, capacity: int = 0):
        from .hasher import default_context

        self.handle = None
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        _capi.check(_capi.lib().oxh_dedup_index_create(self.ctx.handle, int(capacity), ctypes.byref(h)),
                    "oxh_dedup_index_create")
        self.handle = h

    def _live(self):
        if not self.handle:
            raise _capi.OxenError("the dedup index is closed", _capi.OXH_ERR_INVALID)
        return self.handle

    def insert(self, digests, lens=None):
        """digests: (n, 2) uint64 rows of (lo, hi), as FastCdcTable.digests; lens: n chunk lengths or
        None. Returns (first, stats): first[i] (numpy uint64) = the smallest ordinal with row i's
        digest, over everything inserted so far including this call; stats a DedupStats."""
        h = self._live()
        dig = _digest_rows(digests)
        n = dig.shape[0]
        ln = None
        if lens is not None:
            ln = np.ascontiguousarray(lens, dtype=np.uint64)
            if ln.shape != (n,):
                raise _capi.OxenError("lens must hold one length per digest", _capi.OXH_ERR_INVALID)
        first = np.zeros(n, dtype=np.uint64)
        stats = np.zeros(4, dtype=np.uint64)
        _capi.check(_capi.lib().oxh_dedup_index_insert_host(h, dig.ctypes.data_as(_capi._u64p),
                                                            ln.ctypes.data_as(_capi._u64p) if ln is not None else None, n,
                                                            first.ctypes.data_as(_capi._u64p),
                                                            stats.ctypes.data_as(_capi._u64p)), "oxh_dedup_index_insert_host")
        return first, DedupStats(*(int(v) for v in stats))

    def insert_device(self, d_digests: torch.Tensor, d_lens: Optional[torch.Tensor] = None, stream=None):
        """The same over device-resident tensors (digests (n, 2), 64-bit; lens n, 64-bit or None) on
        `stream` (default: the current torch stream). Returns (first, stats), first an int64 device
        tensor holding the raw u64 words. Blocks until complete."""
        from .device import _require_cuda, _stream

        h = self._live()
        _require_cuda(d_digests, *([d_lens] if d_lens is not None else []))
        if d_digests.element_size() != 8 or d_digests.numel() % 2 or not d_digests.is_contiguous():
            raise _capi.OxenError("d_digests must be a contiguous 64-bit (n, 2) tensor", _capi.OXH_ERR_INVALID)
        n = d_digests.numel() // 2
        if d_lens is not None and (d_lens.element_size() != 8 or d_lens.numel() != n or not d_lens.is_contiguous()):
            raise _capi.OxenError("d_lens must be a contiguous 64-bit tensor of one length per digest", _capi.OXH_ERR_INVALID)
        first = torch.empty(n, dtype=torch.int64, device=d_digests.device)
        stats = np.zeros(4, dtype=np.uint64)
        _capi.check(_capi.lib().oxh_dedup_index_insert_device(h, d_digests.data_ptr(),
                                                              d_lens.data_ptr() if d_lens is not None else None, n,
                                                              first.data_ptr(), stats.ctypes.data_as(_capi._u64p),
                                                              _stream(stream)), "oxh_dedup_index_insert_device")
        return first, DedupStats(*(int(v) for v in stats))

    def query(self, digests) -> np.ndarray:
        """first[i] = the ordinal of the first row with that digest, or ABSENT; inserts nothing."""
        h = self._live()
        dig = _digest_rows(digests)
        first = np.zeros(dig.shape[0], dtype=np.uint64)
        _capi.check(_capi.lib().oxh_dedup_index_query_host(h, dig.ctypes.data_as(_capi._u64p), dig.shape[0],
                                                           first.ctypes.data_as(_capi._u64p)), "oxh_dedup_index_query_host")
        return first

    def counts(self) -> DedupCounts:
        out = np.zeros(4, dtype=np.uint64)
        _capi.check(_capi.lib().oxh_dedup_index_counts(self._live(), out.ctypes.data_as(_capi._u64p)),
                    "oxh_dedup_index_counts")
        return DedupCounts(*(int(v) for v in out))

    def close(self) -> None:
        if getattr(self, "handle", None):
            _capi.lib().oxh_dedup_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _own_first(index, digests, lens) -> np.ndarray:
    """Insert a table's rows; True for the rows that are their own first occurrence in the index."""
    base = int(index.counts()[0])
    first, _ = index.insert(digests, lens)
    return np.asarray(first, dtype=np.uint64) == np.arange(base, base + len(first), dtype=np.uint64)


def table_lens(table, chunk_size: Optional[int] = None) -> np.ndarray:
    """Chunk lengths of a table's rows: a FastCdcTable carries them; a FixedChunkTable's follow from
    its files' sizes and the chunk size (every chunk of a file is chunk_size long but the last)."""
    if getattr(table, "lens", None) is not None:
        return np.asarray(table.lens, dtype=np.uint64)
    chunk = int(chunk_size or getattr(table, "chunk_size", None) or 0)
    if chunk <= 0 or table.sizes is None:
        raise _capi.OxenError("a fixed-size table needs its files' sizes and the chunk size", _capi.OXH_ERR_INVALID)
    first = np.asarray(table.first, dtype=np.int64)
    lens = np.full(int(first[-1]), chunk, dtype=np.uint64)
    for i, size in enumerate(np.asarray(table.sizes, dtype=np.uint64).tolist()):
        a, b = int(first[i]), int(first[i + 1])
        if b > a:
            if (size + chunk - 1) // chunk != b - a:
                raise _capi.OxenError(f"file {i}: {b - a} chunks do not cover {size} bytes at {chunk}", _capi.OXH_ERR_INVALID)
            lens[b - 1] = size - (b - a - 1) * chunk
    return lens


def dedup_report(table, index=None, chunk_size: Optional[int] = None) -> dict:
    """The dedup ratio of a chunk table (FastCdcTable / FixedChunkTable): its rows go into `index` (a
    fresh DedupIndex when None) in table order, and a chunk counts as distinct where it is its own
    first occurrence -- so with an index that already holds rows, "distinct" means new to the index,
    and a file's distinct chunks are those no earlier file (or row) carried. Returns
    {"chunks", "distinct_chunks", "bytes", "distinct_bytes", "ratio", "files": [the same per file]};
    ratio = distinct_bytes / bytes (1.0 for no bytes)."""
    lens = table_lens(table, chunk_size)
    own = index is None
    index = DedupIndex() if own else index
    try:
        is_first = _own_first(index, table.digests, lens)
    finally:
        if own:
            index.close()

    def row(a: int, b: int) -> dict:
        total = int(lens[a:b].sum(dtype=np.uint64))
        distinct = int(lens[a:b][is_first[a:b]].sum(dtype=np.uint64))
        return {"chunks": b - a, "distinct_chunks": int(is_first[a:b].sum()), "bytes": total, "distinct_bytes": distinct,
                "ratio": distinct / total if total else 1.0}

    first = np.asarray(table.first, dtype=np.int64)
    out = row(0, len(lens))
    out["files"] = [row(int(first[i]), int(first[i + 1])) for i in range(len(first) - 1)]
    return out


OXH_CHUNK_OVERLAP_MAX_SETS = 256  # include/oxen_hash.h


class ChunkOverlap(NamedTuple):
    """rows[a][b] = the rows of set a, with multiplicity, whose digest occurs in set b (the diagonal is
    set a's row count; not symmetric when a set repeats a digest); bytes the same sum over the rows'
    lengths, None when no lengths were given. Both (nsets, nsets) uint64."""
    rows: np.ndarray
    bytes: Optional[np.ndarray]


def _set_first(counts) -> np.ndarray:
    first = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), out=first[1:])
    return first


def chunk_overlap(sets, lens=None, ctx: Optional[_capi.Context] = None) -> ChunkOverlap:
    """oxh_chunk_overlap_host: how many chunks each set shares with each other set, all pairs in one
    call on the device -- oxendedup.rs:56-70 `count_commit_overlap(c1, c2)` is rows[c1][c2].
    sets: a list of (n_k, 2) uint64 arrays of (lo, hi) rows, or of FastCdcTable / FixedChunkTable
    objects (their lengths come through table_lens); lens: one array of n_k lengths per set, or None."""
    from .hasher import default_context

    digs, lns = [], []
    for k, s in enumerate(sets):
        if hasattr(s, "digests") and hasattr(s, "first"):
            digs.append(_digest_rows(s.digests))
            lns.append(table_lens(s) if lens is None else None)
        else:
            digs.append(_digest_rows(s))
            lns.append(None)
        if lens is not None:
            lns[k] = np.ascontiguousarray(lens[k], dtype=np.uint64)
        if lns[k] is not None and lns[k].shape != (digs[k].shape[0],):
            raise _capi.OxenError(f"set {k}: lens must hold one length per digest", _capi.OXH_ERR_INVALID)
    nsets = len(digs)
    with_lens = nsets > 0 and all(l is not None for l in lns)
    dig = np.concatenate(digs) if nsets else np.zeros((0, 2), dtype=np.uint64)
    ln = np.concatenate(lns) if with_lens else None
    first = _set_first([d.shape[0] for d in digs])
    rows = np.zeros((nsets, nsets), dtype=np.uint64)
    nbytes = np.zeros((nsets, nsets), dtype=np.uint64) if with_lens else None
    # without a device there is no context to make: the library answers OXH_ERR_NODEVICE (after its
    # argument checks, which need neither)
    handle = (ctx or default_context()).handle if ctx is not None or torch.cuda.is_available() else None
    _capi.check(_capi.lib().oxh_chunk_overlap_host(handle, dig.ctypes.data_as(_capi._u64p),
                                         ln.ctypes.data_as(_capi._u64p) if ln is not None else None,
                                         first.ctypes.data_as(_capi._u64p), nsets, rows.ctypes.data_as(_capi._u64p),
                                         nbytes.ctypes.data_as(_capi._u64p) if nbytes is not None else None),
                "oxh_chunk_overlap_host")
    return ChunkOverlap(rows, nbytes)


def chunk_overlap_device(d_digests: torch.Tensor, set_first, d_lens: Optional[torch.Tensor] = None, stream=None,
                         ctx: Optional[_capi.Context] = None) -> ChunkOverlap:
    """oxh_chunk_overlap_device: the same over device-resident tensors (digests (N, 2), 64-bit; lens N,
    64-bit or None) on `stream` (default: the current torch stream); set_first: nsets + 1 host integers,
    set k = rows [set_first[k], set_first[k+1]). The matrices come back in host memory. Blocks."""
    from .device import _require_cuda, _stream
    from .hasher import default_context

    _require_cuda(d_digests, *([d_lens] if d_lens is not None else []))
    if d_digests.element_size() != 8 or d_digests.numel() % 2 or not d_digests.is_contiguous():
        raise _capi.OxenError("d_digests must be a contiguous 64-bit (n, 2) tensor", _capi.OXH_ERR_INVALID)
    n = d_digests.numel() // 2
    if d_lens is not None and (d_lens.element_size() != 8 or d_lens.numel() != n or not d_lens.is_contiguous()):
        raise _capi.OxenError("d_lens must be a contiguous 64-bit tensor of one length per digest", _capi.OXH_ERR_INVALID)
    first = np.ascontiguousarray(set_first, dtype=np.uint64)
    if first.ndim != 1 or first.size < 2 or int(first[-1]) != n:
        raise _capi.OxenError("set_first must hold nsets + 1 entries and end at the row count", _capi.OXH_ERR_INVALID)
    nsets = first.size - 1
    rows = np.zeros((nsets, nsets), dtype=np.uint64)
    nbytes = np.zeros((nsets, nsets), dtype=np.uint64) if d_lens is not None else None
    _capi.check(_capi.lib().oxh_chunk_overlap_device((ctx or default_context()).handle, d_digests.data_ptr() if n else None,
                                                     d_lens.data_ptr() if d_lens is not None and n else None,
                                                     first.ctypes.data_as(_capi._u64p), nsets,
                                                     rows.ctypes.data_as(_capi._u64p),
                                                     nbytes.ctypes.data_as(_capi._u64p) if nbytes is not None else None,
                                                     _stream(stream)), "oxh_chunk_overlap_device")
    return ChunkOverlap(rows, nbytes)


def names_to_digests(names) -> np.ndarray:
    """Decimal u128 chunk names (chunk_name, the strings of get_chunk_hashes) -> (n, 2) uint64 rows of
    (lo, hi): the inverse of chunk_name."""
    out = np.zeros((len(names), 2), dtype=np.uint64)
    for i, name in enumerate(names):
        v = int(name)
        if not 0 <= v < 1 << 128 or str(v) != str(name):
            raise _capi.OxenError(f"{name!r} is not the decimal name of a 128-bit digest", _capi.OXH_ERR_INVALID)
        out[i, 0], out[i, 1] = v & ((1 << 64) - 1), v >> 64
    return out


def count_commit_overlap(commit1, commit2, ctx: Optional[_capi.Context] = None) -> int:
    """oxendedup.rs:56-70: the hashes of commit1, with multiplicity, that commit2 contains -- entry
    [0][1] of one chunk_overlap call instead of a Vec::contains scan per hash."""
    return int(chunk_overlap([names_to_digests(commit1), names_to_digests(commit2)], ctx=ctx).rows[0, 1])


def rust_debug_strings(items) -> str:
    """Rust's `{:?}` of a Vec<String> (the *_hashes.txt files, oxendedup.rs:170-173): `["1", "2"]`."""
    esc = {"\\": "\\\\", '"': '\\"', "\n": "\\n", "\r": "\\r", "\t": "\\t"}
    return "[" + ", ".join('"' + "".join(esc.get(c, c) for c in s) + '"' for s in items) + "]"


# fixedsize.rs:67-91 reads through `BufReader::new(File)` (8 KiB buffer) and stops at the first read
# shorter than chunk_size. BufReader::read serves a request from what is buffered (refilling with one
# 8 KiB read when empty) unless the buffer is empty and the request is >= 8 KiB, which goes to the
# file directly; Linux returns at most MAX_RW_COUNT (0x7ffff000) bytes from one read(2).
BUFREADER_CAPACITY = 8192
MAX_RW_COUNT = 0x7FFFF000


def bufreader_prefix(size: int, chunk: int) -> int:
    """Bytes of a `size`-byte regular file that fixedsize.rs's loop chunks (its chunks are then the
    fixed-size chunks of that prefix): the whole file unless chunk < 8 KiB does not divide 8 KiB (the
    read after the last whole chunk of the first buffer comes back short: the file stops at 8 KiB) or
    chunk > MAX_RW_COUNT (the first read comes back short)."""
    if chunk < BUFREADER_CAPACITY:
        return min(size, BUFREADER_CAPACITY) if BUFREADER_CAPACITY % chunk else size
    return min(size, MAX_RW_COUNT) if chunk > MAX_RW_COUNT else size


class FastCDChunker:
    """fastcdchunker.rs:30-66 + the Chunker trait (chunker.rs): name / pack / unpack / get_chunk_hashes."""

    def __init__(self, chunk_size: int, concurrency: int = 1, device: Optional[str] = None):
        if chunk_size == 0:
            raise ValueError("Chunk size cannot be zero")
        if concurrency == 0:
            raise ValueError("Concurrency must be greater than zero")
        self.min_chunk_size = MIN_CHUNK_SIZE
        self.avg_chunk_size = int(chunk_size)
        self.max_chunk_size = int(chunk_size) * 2
        self.device = device or "cuda"

    def name(self) -> str:
        return "fastcdc-chunker"

    def chunk_buffer(self, data: torch.Tensor):
        """(offsets, lengths, digests) of one device-resident buffer, as numpy uint64 arrays."""
        c_off, c_len, dig, _ = fastcdc_device(data, [0], [data.numel()], self.min_chunk_size, self.avg_chunk_size,
                                              self.max_chunk_size)
        return to_numpy_u64(c_off), to_numpy_u64(c_len), to_numpy_u64(dig).reshape(-1, 2)

    def pack(self, input_file: str, output_dir: str, ctx: Optional[_capi.Context] = None, index=None) -> str:
        """fastcdchunker.rs:72-122. The library reads the file (oxh_fastcdc_files: its bytes stream to
        the device once; boundaries and chunk digests come back to host memory); the chunk files are
        then written from a read-only map of the input, as the reference writes its slices.
        index (a DedupIndex that belongs to this output_dir: every row ever inserted into it is a chunk
        file there): the table is inserted and only the rows that are their own first occurrence are
        written -- the directory ends up the same, without the rewrites of repeated chunks."""
        import errno as _errno
        import mmap

        os.makedirs(output_dir, exist_ok=True)
        tab = fastcdc_files([input_file], self.min_chunk_size, self.avg_chunk_size, self.max_chunk_size, ctx=ctx)
        if int(tab.status[0]) != _capi.OXH_OK:  # fs::read(input_file)? (:75): the io::Error
            e = int(tab.os_error[0]) or _errno.EIO
            raise OSError(e, os.strerror(e), input_file)
        size = os.stat(input_file).st_size  # input_file.metadata()?.len() (:77-78)
        names = []
        wanted = _own_first(index, tab.digests, tab.lens).tolist() if index is not None else None
        with open(input_file, "rb") as fh:
            content = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if size else b""
            try:
                for k, (o, l, (lo, hi)) in enumerate(zip(tab.offsets, tab.lens, tab.digests)):
                    name = chunk_name(lo, hi)
                    names.append(name)
                    if wanted is not None and not wanted[k]:
                        continue
                    with open(os.path.join(output_dir, name), "wb") as out:
                        out.write(content[int(o):int(o) + int(l)])
            finally:
                if size:
                    content.close()
        base = os.path.basename(os.path.normpath(input_file)) or "unknown_file"
        with open(os.path.join(output_dir, METADATA_FILE_NAME), "wb") as meta:
            meta.write(encode_metadata(base, size, names))
        return output_dir

    def unpack(self, input_dir: str, output_path: str) -> str:
        """fastcdchunker.rs:123-126: the reference's unpack is a stub -- it prints and returns
        output_path without writing anything (so its `Test` command fails to hash the unpacked file).
        Kept as such; `restore` is the working inverse."""
        print(f"To Implement: Unpacking files from {input_dir!r}")
        return output_path

    def restore(self, input_dir: str, output_path: str) -> str:
        """Not in the reference: concatenate the chunks listed in metadata.bin into output_path."""
        _, _, chunks = decode_metadata(open(os.path.join(input_dir, METADATA_FILE_NAME), "rb").read())
        with open(output_path, "wb") as out:
            for c in chunks:
                with open(os.path.join(input_dir, c), "rb") as fh:
                    out.write(fh.read())
        return output_path

    def get_chunk_hashes(self, input_dir: str) -> list[str]:
        return decode_metadata(open(os.path.join(input_dir, METADATA_FILE_NAME), "rb").read())[2]


class _FixedSizeBase:
    """Shared by both fixed-size chunkers: a file -> its chunk names, chunks written as they are named."""

    def __init__(self, chunk_size: int, concurrency: int = 1, device: Optional[str] = None):
        if chunk_size == 0:
            raise ValueError("Chunk size cannot be zero")
        if concurrency == 0:
            raise ValueError("Concurrency must be greater than zero")
        self.chunk_size = int(chunk_size)
        self.concurrency = int(concurrency)
        self.device = device or "cuda"

    def _prefix(self, size: int) -> int:
        """Bytes of the file the reference chunks (all of them; FixedSizeChunker overrides)."""
        return size

    def chunk_file(self, path: str, output_dir: str, index=None) -> list[str]:
        """Decimal xxh3_128 names of the file's chunks; a chunk file is written unless one of that
        name exists (fixedsize.rs:78-89, fixedsize_multithreaded.rs:95-105). The library reads the file
        and returns the digests (oxh_chunk_digests_files); the chunk files are written from a read-only
        map of it by `concurrency` threads.
        index (a DedupIndex that belongs to this output_dir: every row ever inserted into it is a chunk
        file there): the digests are inserted and only the rows that are their own first occurrence
        are looked at; the others cost no `exists` call."""
        import errno as _errno
        import mmap
        from concurrent.futures import ThreadPoolExecutor

        size = os.stat(path).st_size
        pre = self._prefix(size)
        if pre == size:
            tab = chunk_digests_files([path], self.chunk_size)
            if int(tab.status[0]) != _capi.OXH_OK:  # File::open / read: the io::Error
                e = int(tab.os_error[0]) or _errno.EIO
                raise OSError(e, os.strerror(e), path)
            size = int(tab.sizes[0])
            dig = tab.digests
        else:  # the reference's loop stops early: chunk the prefix it reads
            with open(path, "rb") as fh:
                head = fh.read(pre)
            dig = chunk_digests_host([head], self.chunk_size).digests
        names = [chunk_name(lo, hi) for lo, hi in dig.tolist()]
        if not names:
            return names
        rows = range(len(names))
        if index is not None:
            starts = np.arange(len(names), dtype=np.uint64) * np.uint64(self.chunk_size)
            lens = np.minimum(starts + np.uint64(self.chunk_size), np.uint64(pre)) - starts
            rows = np.nonzero(_own_first(index, dig, lens))[0].tolist()
        with open(path, "rb") as fh:
            content = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
            try:
                def write(k):
                    p = os.path.join(output_dir, names[k])
                    if not os.path.exists(p):
                        lo = k * self.chunk_size
                        with open(p, "wb") as out:
                            out.write(content[lo:min(pre, lo + self.chunk_size)])

                with ThreadPoolExecutor(self.concurrency) as ex:
                    list(ex.map(write, rows))
            finally:
                content.close()
        return names


class FixedSizeChunker(_FixedSizeBase):
    """fixedsize.rs:37-296 + the Chunker trait: packs a file or a whole directory tree (entries in
    read_dir order, a directory's entry before its contents) into chunk files + ArchiveMetadata."""

    def __init__(self, chunk_size: int, device: Optional[str] = None):
        super().__init__(chunk_size, 1, device)

    def name(self) -> str:
        return "fixed-size-chunker"

    def _prefix(self, size: int) -> int:
        return bufreader_prefix(size, self.chunk_size)

    def _file_entry(self, path: str, base: str, output_dir: str, index=None) -> dict:
        chunks = self.chunk_file(path, output_dir, index)
        return {"path": os.path.relpath(path, base), "is_dir": False, "chunks": chunks, "size": os.stat(path).st_size}

    def _walk(self, cur: str, base: str, output_dir: str, entries: list, index=None) -> None:
        with os.scandir(cur) as it:  # read_dir order (fixedsize.rs:116)
            for e in it:
                if e.is_dir():  # metadata() follows symlinks, as here
                    entries.append({"path": os.path.relpath(e.path, base), "is_dir": True, "chunks": None, "size": None})
                    self._walk(e.path, base, output_dir, entries, index)
                elif e.is_file():
                    entries.append(self._file_entry(e.path, base, output_dir, index))

    def pack(self, input_path: str, output_dir: str, index=None) -> str:
        """index: a DedupIndex that belongs to output_dir (chunk_file)."""
        os.makedirs(output_dir, exist_ok=True)
        entries: list = []
        if os.path.isfile(input_path):
            base = os.path.dirname(os.path.abspath(input_path))
            entries.append(self._file_entry(os.path.abspath(input_path), base, output_dir, index))
        elif os.path.isdir(input_path):
            entries.append({"path": ".", "is_dir": True, "chunks": None, "size": None})
            self._walk(input_path, input_path, output_dir, entries, index)
        else:
            raise _capi.OxenError("Input path must be a file or a directory", _capi.OXH_ERR_INVALID)
        with open(os.path.join(output_dir, METADATA_FILE_NAME), "wb") as f:
            f.write(encode_archive_metadata(self.chunk_size, entries))
        return output_dir

    def unpack(self, chunk_dir: str, output_dir: str) -> str:
        _, entries = decode_archive_metadata(open(os.path.join(chunk_dir, METADATA_FILE_NAME), "rb").read())
        os.makedirs(output_dir, exist_ok=True)
        for e in entries:
            out = os.path.join(output_dir, e["path"])
            if e["is_dir"]:
                os.makedirs(out, exist_ok=True)
                continue
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "wb") as fh:
                for c in e["chunks"] or []:
                    p = os.path.join(chunk_dir, c)
                    if not os.path.exists(p):
                        raise FileNotFoundError(f"Chunk file not found during unpack: {p}")
                    with open(p, "rb") as ch:
                        fh.write(ch.read())
        return output_dir

    def get_chunk_hashes(self, input_dir: str) -> list[str]:
        _, entries = decode_archive_metadata(open(os.path.join(input_dir, METADATA_FILE_NAME), "rb").read())
        return [c for e in entries if not e["is_dir"] for c in (e["chunks"] or [])]


class FixedSizeMultiChunker(_FixedSizeBase):
    """fixedsize_multithreaded.rs:24-245 (the reference's rayon pool of `concurrency`): one file ->
    chunk files + ChunkMetadata {original_file_name, original_file_size, chunk_size, chunks}."""

    def name(self) -> str:
        return "fixed-size-64k-multithreaded"

    def pack(self, input_file: str, output_dir: str, index=None) -> str:
        """index: a DedupIndex that belongs to output_dir (chunk_file)."""
        os.makedirs(output_dir, exist_ok=True)
        try:
            size = os.stat(input_file).st_size
        except OSError as e:
            raise FileNotFoundError(f"Failed to read input file metadata '{input_file}': {e}") from e
        names = self.chunk_file(input_file, output_dir, index) if size else []
        base = os.path.basename(os.path.normpath(input_file)) or "unknown_file"
        with open(os.path.join(output_dir, METADATA_FILE_NAME), "wb") as f:
            f.write(encode_fixed_metadata(base, size, self.chunk_size, names))
        return output_dir

    def unpack(self, chunk_dir: str, output_path: str) -> str:
        _, _, _, chunks = decode_fixed_metadata(open(os.path.join(chunk_dir, METADATA_FILE_NAME), "rb").read())
        with open(output_path, "wb") as out:
            for c in chunks:
                p = os.path.join(chunk_dir, c)
                if not os.path.exists(p):
                    raise FileNotFoundError(f"Chunk file not found during unpack: {p}")
                with open(p, "rb") as fh:
                    out.write(fh.read())
        return output_path

    def get_chunk_hashes(self, input_dir: str) -> list[str]:
        return decode_fixed_metadata(open(os.path.join(input_dir, METADATA_FILE_NAME), "rb").read())[3]


def get_chunker(algorithm: str, chunk_size: int):
    """chunker.rs:60-124 get_chunker: "fixed-size", "fixed-size-multithreaded" (16 threads) and
    "fastcdc" (the "copier" baseline copies files and hashes nothing: not on this path)."""
    if algorithm == "fixed-size":
        return FixedSizeChunker(chunk_size)
    if algorithm == "fixed-size-multithreaded":
        return FixedSizeMultiChunker(chunk_size, 16)
    if algorithm == "fastcdc":
        return FastCDChunker(chunk_size, 16)
    raise _capi.OxenError(f"Chunker '{algorithm}' not found", _capi.OXH_ERR_INVALID)


VERSION_FILE_NAME = "data"  # oxendedup.rs:14


class OxenChunker:
    """oxendedup.rs:27-218, behind main.rs's `TestOxen`: pack one file's version blob in each of the n
    latest commits and say how many chunks each version shares with the one before it."""

    def __init__(self, chunk_size: int, chunk_algorithm: str, root_path):
        self.chunk_size = int(chunk_size)
        self.chunk_algorithm = str(chunk_algorithm)
        self.root_path = os.fspath(root_path)

    def version_dir(self, file_hash: str) -> str:
        """oxendedup.rs:46-50: root/{hash[..2]}/{hash[2..]}."""
        return os.path.join(self.root_path, file_hash[:2], file_hash[2:])

    def version_path(self, file_hash: str) -> str:
        """oxendedup.rs:52-54."""
        return os.path.join(self.version_dir(file_hash), VERSION_FILE_NAME)

    def pack(self, algo: str, chunk_size: int, versions, output_dir, n: Optional[int] = None,
             ctx: Optional[_capi.Context] = None) -> dict:
        """oxendedup.rs:72-209. versions: (commit_id, file_hash_hex or None) per commit, newest first --
        what `commits::list` and `tree::get_file_by_path` give the reference (Oxen's commit and merkle
        stores are not read here); the first n are used. Every present version is packed with
        get_chunker(algo, chunk_size) into output_dir/<commit_id>; for every k >= 1 commit k's directory
        gets <commit_{k-1}>_hashes.txt and <commit_k>_hashes.txt (`{:?}` of the chunk names). All overlaps
        come from ONE chunk_overlap call over every version's get_chunk_hashes, where the reference runs
        count_commit_overlap pair by pair. Returns {"commits", "matrix": ChunkOverlap, "pairs": [{"commit1",
        "commit2", "overlap", "commit1_chunks", "commit2_chunks"}]}. No versions: ValueError (the
        reference indexes [0]); a pair with a missing version: FileNotFoundError, as the reference's `?`."""
        output_dir = os.fspath(output_dir)
        latest = list(versions)[:n] if n is not None else list(versions)
        if not latest:
            raise ValueError("no commits to pack")
        os.makedirs(output_dir, exist_ok=True)
        chunker = get_chunker(algo, chunk_size)
        commits = [str(c) for c, _ in latest]
        hashes: list[list[str]] = []

        def chunk_hashes(commit: str) -> list[str]:
            try:
                return chunker.get_chunk_hashes(os.path.join(output_dir, commit))
            except FileNotFoundError as e:
                raise FileNotFoundError(f"error getting chunk hashes for hash {commit} : {e}") from e

        for k, (commit, file_hash) in enumerate(zip(commits, (h for _, h in latest))):
            commit_dir = os.path.join(output_dir, commit)
            os.makedirs(commit_dir, exist_ok=True)
            if file_hash is not None:
                chunker.pack(self.version_path(str(file_hash)), commit_dir)
            else:
                print(f"No file found for commit: {commit!r}")
            if k >= 1:
                if len(hashes) < k:
                    hashes.append(chunk_hashes(commits[k - 1]))  # commit 0's, read with its first pair
                hashes.append(chunk_hashes(commit))
                for name, names in ((commits[k - 1], hashes[k - 1]), (commit, hashes[k])):
                    with open(os.path.join(commit_dir, f"{name}_hashes.txt"), "w") as fh:
                        fh.write(rust_debug_strings(names))
        if not hashes:  # n == 1: no pair, and a missing version is no error
            try:
                hashes.append(chunk_hashes(commits[0]))
            except FileNotFoundError:
                hashes.append([])
        matrix = chunk_overlap([names_to_digests(h) for h in hashes], ctx=ctx)
        pairs = [{"commit1": commits[k - 1], "commit2": commits[k], "overlap": int(matrix.rows[k - 1, k]),
                  "commit1_chunks": len(hashes[k - 1]), "commit2_chunks": len(hashes[k])} for k in range(1, len(commits))]
        for p in pairs:  # oxendedup.rs:184-197
            if p["overlap"] > 0:
                print(f"Commit {p['commit1']} and {p['commit2']} have {p['overlap']} overlapping chunks out of "
                      f"{p['commit1_chunks']}")
            else:
                print(f"Commit {p['commit1']} and {p['commit2']} have no overlapping chunks")
        return {"commits": commits, "matrix": matrix, "pairs": pairs}

    def unpack(self, input_dir, output_file):
        """oxendedup.rs:211-217: the reference's stub -- it prints and returns output_file."""
        print(f"Unpacking repository data with content-defined chunking... {os.fspath(input_dir)}")
        return output_file


def fastcdc_gear() -> list[int]:
    """The GEAR table compiled into the library (host call, no GPU needed)."""
    out = np.zeros(256, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_fastcdc_gear(out.ctypes.data_as(_capi._u64p)), "oxh_fastcdc_gear")
    return [int(v) for v in out]


def fastcdc_masks(avg_size: int, level: int = 1) -> tuple[int, int]:
    s = np.zeros(1, dtype=np.uint64)
    l = np.zeros(1, dtype=np.uint64)
    _capi.check(_capi.lib().oxh_fastcdc_masks(int(avg_size), int(level), s.ctypes.data_as(_capi._u64p),
                                              l.ctypes.data_as(_capi._u64p)), "oxh_fastcdc_masks")
    return int(s[0]), int(l[0])


def hash_file_128bit(path) -> int:
    """xhash.rs:6-20: File::open, 8 KiB BufReader reads into Xxh3, digest128 -- the XXH3-128 of the
    whole file, here read and hashed by the library (oxh_hash_files_ex). The io::Error of the open /
    read comes back as OSError."""
    import errno as _errno

    from .hasher import hash_files_with_errors_128bit

    digests, _, status, oserr = hash_files_with_errors_128bit([os.fspath(path)])
    if status[0] != _capi.OXH_OK:
        e = int(oserr[0]) or _errno.EIO
        raise OSError(e, os.strerror(e), os.fspath(path))
    return int(digests[0])


class VerificationFailed(Exception):
    """FrameworkError::VerificationFailed (main.rs:232-234)."""


def run_chunker_test(algorithm: str, chunk_size: int, input_file: str, base_dir: Optional[str] = None) -> dict:
    """main.rs:156-241, `Commands::Test`: pack input_file into base_dir/chunker_test_<ns>, unpack it to
    <that dir>/unpacked_output, time both, then compare hash_file_128bit of the original and of the
    unpacked file (VerificationFailed when they differ; a failed hash is "Failed to hash ... file")."""
    import time

    chunker = get_chunker(algorithm, chunk_size)
    base = base_dir if base_dir is not None else os.getcwd()
    test_dir = os.path.join(base, f"chunker_test_{time.time_ns()}")
    os.makedirs(test_dir, exist_ok=True)
    t0 = time.perf_counter()
    chunker.pack(input_file, test_dir)
    pack_s = time.perf_counter() - t0
    unpacked = os.path.join(test_dir, "unpacked_output")
    t0 = time.perf_counter()
    chunker.unpack(test_dir, unpacked)
    unpack_s = time.perf_counter() - t0
    try:
        original = hash_file_128bit(input_file)
    except OSError as e:
        raise _capi.OxenError(f"Failed to hash original file: {e}", _capi.OXH_ERR_IO) from e
    try:
        restored = hash_file_128bit(unpacked)
    except OSError as e:
        raise _capi.OxenError(f"Failed to hash unpacked file: {e}", _capi.OXH_ERR_IO) from e
    if original != restored:
        raise VerificationFailed("Verification FAILED: Unpacked file does NOT match original.")
    return {"test_dir": test_dir, "pack_s": pack_s, "unpack_s": unpack_s, "original_file_hash": str(original)}
