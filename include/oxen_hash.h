/*
 * include/oxen_hash.h -- C ABI of the MI355X content-hashing stage for `oxen add` / commit.
 *
 * Drop-in boundary for liboxen's `util::hasher` module (crates/liboxen/src/util/hasher.rs) and the
 * per-file hash call in the add loop (crates/liboxen/src/core/v_latest/add.rs:716-718,741-743).
 * Every digest is XXH3-128 with seed 0 and the default secret -- bit-identical to
 * `xxhash_rust::xxh3::xxh3_128` (xxhash-rust 0.8.15) -- returned as two u64 words per item:
 * out[2*i] = low 64 bits, out[2*i+1] = high 64 bits, i.e. the Rust `u128` is
 * `((hi as u128) << 64) | lo as u128` (MerkleHash, model/merkle_tree/merkle_hash.rs:16).
 *
 * Conventions:
 *   - plain pointers and sizes only; no torch / Rust / HIP-runtime types in the signatures
 *     (`stream` is an opaque hipStream_t; NULL = the null stream, as in HIP itself);
 *   - every function returns an int status (OXH_OK == 0); batch calls also fill a per-item
 *     `status[]` so one unreadable file never fails the batch (add.rs:533-544 logs and skips);
 *   - the library never frees caller memory and retains no caller pointer after returning;
 *   - all entry points are thread-safe; file calls on one context are requests to the context's
 *     streaming engine, and concurrent ones share its live pipeline (each caller returns when its
 *     own files are done); other calls on a context serialise;
 *   - there is no CPU fallback: without a usable gfx950 device, calls fail with OXH_ERR_NODEVICE.
 *
 * The Rust-side `extern "C"` block that binds these is in INTEGRATION.md.
 */
#ifndef OXEN_HASH_H
#define OXEN_HASH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OXH_ABI_VERSION 5

/* status codes (also used per item in status[]) */
#define OXH_OK 0
#define OXH_ERR_INVALID 1   /* bad argument */
#define OXH_ERR_HIP 2       /* HIP runtime error */
#define OXH_ERR_IO 3        /* file opened but its read failed (hasher.rs:135-139, 162-165) */
#define OXH_ERR_NOMEM 4     /* host or device allocation failed */
#define OXH_ERR_NODEVICE 5  /* no usable MI355X (gfx950) device */
#define OXH_ERR_OPEN 7      /* per item: File::open failed (hasher.rs:141-145, 151-154) */

/* kernel selection for the device-resident batch */
#define OXH_MODE_AUTO 0     /* one wave per buffer (K1), lane-per-item for short-only batches */
#define OXH_MODE_WAVE 1     /* force K1: one 64-lane wave per buffer */
#define OXH_MODE_LANE 2     /* force K1s: one lane per buffer (short items, parent-node streams) */
#define OXH_MODE_WAVE_SHORT 3 /* K1 shaped for items of <= ~16 KiB (more resident waves) */
#define OXH_MODE_WAVE_PACKED 4 /* K1 shaped for items packed back to back at arbitrary byte offsets
                                  (FastCDC chunks of one buffer): each wave-instruction reads a
                                  whole 1 KiB block */

typedef struct oxh_ctx oxh_ctx;

/* ---------------------------------------------------------------- library / context */
int oxh_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* oxh_last_error(void);
/* Number of visible HIP devices (0 on a host without a GPU). */
int oxh_device_count(int* count);
/* Create a hashing context on `device`: owns a compute stream, a copy stream, pinned host staging
 * (`staging_bytes` per slot, 0 = default 256 MiB, 3 slots) and matching device slots.
 * staging_bytes above OXH_MAX_STAGING_BYTES fails with OXH_ERR_INVALID (a slot's fill state is one
 * 64-bit word: 31 bits of byte offset, 19 bits of item count at one item per 4 KiB). Files of a
 * slot's size or larger are streamed through the large-file path whatever the setting. */
#define OXH_MAX_STAGING_BYTES 2147483392ull /* 2 GiB - 256 */
int oxh_ctx_create(int device, uint64_t staging_bytes, oxh_ctx** out);
int oxh_ctx_destroy(oxh_ctx* ctx);
/* The context's compute stream (hipStream_t), for callers that want to order against it. */
void* oxh_ctx_stream(oxh_ctx* ctx);

/* ---------------------------------------------------------------- K1 / K1s: device-resident batch
 * Replaces N calls of `hash_buffer_128bit(&[u8]) -> u128` (hasher.rs:28-30) over buffers that are
 * already resident in HBM: item i is d_arena[d_offsets[i] .. d_offsets[i] + d_lens[i]).
 * d_offsets / d_lens / d_out are device pointers; d_out receives 2*n u64. Asynchronous on `stream`.
 * Any start offset and length; starts off a dword boundary are loaded dword-aligned and re-aligned
 * in registers. `mode` (OXH_MODE_*) only picks the kernel shape, never the result: AUTO / WAVE for
 * items placed at 128-B (or coarser) aligned offsets, WAVE_SHORT when they are mostly <= 16 KiB,
 * WAVE_PACKED for items packed back to back at arbitrary offsets (chunks of one buffer). */
int oxh_xxh3_128_batch_device(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens,
                              uint64_t n, uint64_t* d_out, int mode, void* stream);

/* Fixed-size chunk digests of one device-resident buffer (block-level dedup,
 * experiments/block-level-dedup/src/chunker/fixedsize.rs:52-102): chunk i is
 * d_buf[i*chunk .. min((i+1)*chunk, len)); d_out receives 2*ceil(len/chunk) u64. */
int oxh_chunk_digests_device(const void* d_buf, uint64_t len, uint64_t chunk, uint64_t* d_out,
                             void* stream);

/* K1L: whole-buffer digest of one large device-resident buffer (files >= 1e9 B take the streamed
 * branch in hasher.rs:150-174; the digest is the same XXH3-128). Block sums are computed in
 * parallel across the chip, then the serial scramble chain runs on one wave. `d_out` gets 2 u64. */
int oxh_xxh3_128_large_device(oxh_ctx* ctx, const void* d_buf, uint64_t len, uint64_t* d_out,
                              void* stream);

/* K1L over n large device-resident buffers (e.g. the 16 x 8 GiB files of the dedup experiment):
 * d_bufs and lens are HOST arrays of n device pointers / lengths; d_out (device) gets 2n u64.
 * Buffers are processed in rounds of 1 GiB pieces: a round's block sums run chip-wide on `stream`
 * while the previous round's serial chains (up to 32 per launch, resumed from piece to piece) run
 * on a second stream. The block sums live in one of the device's two cached scratch buffers, so
 * both K1L calls return only after `stream` has finished them (a third concurrent caller on the
 * device waits for a buffer). */
int oxh_xxh3_128_large_batch_device(const void* const* d_bufs, const uint64_t* lens, uint64_t n,
                                    uint64_t* d_out, void* stream);

/* ---------------------------------------------------------------- streaming XXH3
 * xxhash-rust's `Xxh3` (new / update / digest128) as used by hasher.rs:73-76, 157-173 (large files),
 * HashingReader / HashingWriter (hasher.rs:183-244) and AtomicFile's verify (atomic_file.rs:396-431).
 * Bytes collect in a pinned buffer; every 16 MiB (OXH_STREAM_PIECE_MIB) of whole 1 KiB blocks go to
 * the device as one K1L piece whose chain resumes from the stream's accumulators, so memory stays
 * bounded whatever the length. digest (2 u64, lo then hi) = xxh3_128 of everything updated so far
 * and leaves the state unchanged. A stream is used by one thread at a time (like `&mut Xxh3`). */
typedef struct oxh_xxh3_stream oxh_xxh3_stream;
int oxh_xxh3_stream_create(oxh_ctx* ctx, oxh_xxh3_stream** out);
int oxh_xxh3_stream_update(oxh_xxh3_stream* s, const void* data, uint64_t len);
int oxh_xxh3_stream_digest(oxh_xxh3_stream* s, uint64_t* out2);
int oxh_xxh3_stream_reset(oxh_xxh3_stream* s);
int oxh_xxh3_stream_destroy(oxh_xxh3_stream* s);

/* ---------------------------------------------------------------- host-resident entry points
 * These block until the digests are in host memory. */

/* hash_buffer_128bit x n over host buffers (pinned staging, H2D on a side stream, K1, D2H). */
int oxh_hash_buffers(oxh_ctx* ctx, const uint8_t* const* bufs, const uint64_t* lens, uint64_t n,
                     uint64_t* out);

/* get_hash_given_metadata / u128_hash_file_contents x n (hasher.rs:56-65,102-112): reads each file
 * whole (parallel readers straight into pinned staging), overlaps H2D with hashing, and returns
 * digests, file sizes and a per-file status (OXH_OK; OXH_ERR_OPEN for a file whose open() fails --
 * File::open in hash_small_file_contents, hasher.rs:141-145; OXH_ERR_IO for a file that opens but
 * cannot be read -- read_to_end, hasher.rs:135-139, e.g. a directory (EISDIR); OXH_ERR_NOMEM for a
 * file larger than a staging slot whose device / pinned buffers cannot be allocated -- the other
 * files of the call are unaffected; digest 0 on error). Files are read to EOF: one whose size
 * differs from its stat (or, below, from the caller's size) is re-read, so the digest covers what
 * the read returned, like read_to_end (hasher.rs:126-148).
 * A call of at most 8 files and 2 MiB on a context with no file request in flight runs on the caller's
 * thread (the same reads and kernels, no engine hand-offs; the thread's current HIP device is restored
 * before return); other calls are requests to the context's engine thread. Either way the results are
 * the same. `sizes` and `status` may be NULL. oxh_hash_files_ex also returns the errno of each failure. */
int oxh_hash_files(oxh_ctx* ctx, const char* const* paths, uint64_t n, uint64_t* out,
                   uint64_t* sizes, int32_t* status);

/* get_hash_given_metadata(path, &metadata) x n (hasher.rs:56-65) with the sizes the caller already
 * holds from its directory walk (add.rs stats every entry): readers skip the fstat and read
 * meta_sizes[i] + 1 bytes; a file whose size differs from meta_sizes[i] is re-read (fstat + whole
 * read), so digests always cover the file's current content. `sizes` returns the sizes read. */
int oxh_hash_files_meta(oxh_ctx* ctx, const char* const* paths, const uint64_t* meta_sizes, uint64_t n,
                        uint64_t* out, uint64_t* sizes, int32_t* status);

/* The add loop's hash and version-store copy, fused (add.rs:507-516, 718, 743;
 * storage/local.rs:104-121; util/fs/atomic_file.rs:363-463): each file is read ONCE into pinned
 * staging and hashed by K1; when its blob is not already in the store it is written from the same
 * pinned bytes to {versions_root}/{hex[..2]}/{hex[2..]}/data (hex = unpadded {:x}) through
 * AtomicTempFile's protocol (util/fs/atomic_file.rs:54-159): a `data.oxentmp.<random>` sibling,
 * data made durable, rename, rename made durable -- with one syncfs() per drained staging slot in
 * place of an fsync per file and per parent. Files larger than a staging slot are streamed: each
 * piece goes to the device and to a temp file in {versions_root} as it is read, and the temp is
 * renamed into place once the digest is known (host memory stays bounded by the bounce buffers).
 * The reference reads a new file three times and hashes it twice (verify-before-publish); here the
 * published bytes are the hashed bytes, so the check holds by construction.
 * Identical content in several items is published once. stored[i] = 1 for the first item of a content
 * whose blob this call wrote, 0 otherwise. status[i] = OXH_ERR_IO (digest 0) for an unreadable file AND for every item
 * whose content could not be published, OXH_ERR_NOMEM as for oxh_hash_files. */
int oxh_add_files(oxh_ctx* ctx, const char* const* paths, uint64_t n, const char* versions_root,
                  uint64_t* out, uint64_t* sizes, int32_t* status, int32_t* stored);
/* oxh_add_files plus os_error[i] as in oxh_hash_files_ex (0 for a failed publish). */
int oxh_add_files_ex(oxh_ctx* ctx, const char* const* paths, uint64_t n, const char* versions_root,
                     uint64_t* out, uint64_t* sizes, int32_t* status, int32_t* stored, int32_t* os_error);

/* Bulk re-hash of a version store: LocalVersionStore::clean_corrupted_versions
 * (storage/local.rs:417-610, `oxen fsck`). Walks {versions_root}/{prefix}/{suffix}/data, hashes every
 * blob on the GPU (files batched exactly as oxh_hash_files) and compares the unpadded hex digest with
 * prefix+suffix. Corrupted or unreadable blobs have their {suffix} directory removed unless dry_run.
 * result[4] = {scanned, corrupted, cleaned, errors} -- the fields of CleanCorruptedVersionsResult
 * (view/versions.rs), counted with the reference's rules: a non-directory under the root is an
 * error; a non-directory under a prefix is skipped; an unreadable blob is an error (not scanned) and
 * is removed unless dry_run; a failed removal is an error. */
int oxh_clean_corrupted_versions(oxh_ctx* ctx, const char* versions_root, int dry_run, uint64_t* result);

/* ---------------------------------------------------------------- reader-process pool
 * oxh_hash_files / oxh_hash_files_meta over a list split across `procs` helper PROCESSES. The warm
 * page-cache floor of reading many small files is open()+close() themselves, and it is per process
 * (200 000 opens: 0.28 s in one process at any thread count, 0.16 s in two, 0.13 s in four;
 * DESIGN.md §5), so one context's engine -- one process -- sits on it. The pool starts helper
 * processes (posix_spawn of `oxh_hash_helper` from this library's directory, $OXH_HELPER overrides),
 * each with its own context on devices[p % ndevices] and `threads` reader threads (<= 0: the
 * process's CPU quota / procs, at most 16); ndevices = 0 means device 0. With devices {0..7} every
 * GPU of a node is fed its own contiguous share over its own PCIe link. Shares are
 * balanced by bytes when meta_sizes is given. Paths and outputs cross the process boundary through
 * one shared-memory region; calls on one pool serialise. Helpers exit on oxh_pool_destroy, or when
 * the creating process exits (whichever thread created the pool: a helper watches its socket and its
 * parent process, not the creating thread). A helper that dies makes the call, and every later call,
 * fail with OXH_ERR_HIP. A helper that is alive but has not answered within OXH_WAIT_LIMIT_S seconds
 * (default 60) is only reported on stderr (the call keeps waiting: a large batch may take that long);
 * OXH_POOL_CALL_LIMIT_S > 0 is the opt-in deadline after which the call, and every later call, fail
 * with OXH_ERR_HIP (default 0 = no deadline). Creation fails with the first helper's error (e.g. OXH_ERR_NODEVICE without a GPU).
 * Replaces the reference's fan-out of 64-file batches over num_cpus*2 tasks of one process
 * (core/v_latest/add.rs:422-425) with a fan-out over processes and devices. */
typedef struct oxh_pool oxh_pool;
int oxh_pool_create(const int* devices, int ndevices, int procs, int threads, uint64_t staging_bytes, oxh_pool** out);
/* oxh_hash_files (meta_sizes == NULL) or oxh_hash_files_meta semantics, per-file status[] included. */
int oxh_pool_hash_files(oxh_pool* pool, const char* const* paths, const uint64_t* meta_sizes, uint64_t n,
                        uint64_t* out, uint64_t* sizes, int32_t* status);
/* oxh_pool_hash_files plus os_error[i] as in oxh_hash_files_ex. */
int oxh_pool_hash_files_ex(oxh_pool* pool, const char* const* paths, const uint64_t* meta_sizes, uint64_t n,
                           uint64_t* out, uint64_t* sizes, int32_t* status, int32_t* os_error);
/* procs = number of helpers; pids (may be NULL) receives their process ids. */
int oxh_pool_size(oxh_pool* pool, int* procs, int* pids);
/* Not while another thread is inside a call on the same pool (the caller owns the pool's lifetime,
 * as with oxh_ctx_destroy). */
int oxh_pool_destroy(oxh_pool* pool);

/* Text-metadata fusion (K1T): the same digests as oxh_hash_files plus, per file, the counts liboxen's
 * text metadata reads in a second full pass (repositories/metadata/text.rs:11-20 ->
 * util/fs.rs:217-263): counts[2i] = num_lines (1 + number of b'\n'), counts[2i+1] = num_chars
 * (bytes that are not UTF-8 continuation bytes, bytecount::num_chars). Computed in the hash's
 * HBM pass; the caller uses them only for files it classifies as text. */
int oxh_hash_files_text(oxh_ctx* ctx, const char* const* paths, uint64_t n, uint64_t* out,
                        uint64_t* sizes, int32_t* status, uint64_t* counts);
/* K1T + the data-type sniff: as oxh_hash_files_text, plus is_utf8[i] = util::fs::is_utf8 of file i
 * (util/fs.rs:652-668: its first min(size, 4096) bytes are UTF-8, or the first error is a sequence cut
 * off by the end of that prefix; 0 for unreadable files), computed on the same staged bytes -- the
 * mime/data-type decision of add.rs:809-810 then needs no third read of the file. */
int oxh_hash_files_text_utf8(oxh_ctx* ctx, const char* const* paths, uint64_t n, uint64_t* out,
                             uint64_t* sizes, int32_t* status, uint64_t* counts, int32_t* is_utf8);
/* The four calls above in one, with the OS error of every failed item: meta_sizes NULL ->
 * oxh_hash_files, else oxh_hash_files_meta semantics; counts non-NULL -> the K1T counts; is_utf8
 * non-NULL (needs counts) -> the sniff. os_error[i] (may be NULL) = the errno of item i's failed open
 * (status OXH_ERR_OPEN) or read (OXH_ERR_IO; 0 when the file ended before the size it was read at),
 * 0 otherwise -- what the io::Error in the reference's message carries: a Rust caller builds
 * `std::io::Error::from_raw_os_error(os_error[i])` and formats hasher.rs's own text with it. */
int oxh_hash_files_ex(oxh_ctx* ctx, const char* const* paths, const uint64_t* meta_sizes, uint64_t n,
                      uint64_t* out, uint64_t* sizes, int32_t* status, int32_t* os_error,
                      uint64_t* counts, int32_t* is_utf8);

/* The modified check of `oxen status` (core/v_latest/status.rs:710,734), add (add.rs:723) and
 * checkout (branches.rs:524,548): util::fs::classify_modified_from_node_with_metadata
 * (util/fs.rs:1580-1619) x n, behind LocalRepository::is_modified_from_node_with_metadata
 * (model/repository/local_repository.rs:601-615). Per item, from the caller's walk: sizes[i] =
 * metadata.len(), node_bytes[i] = node.num_bytes(), mtime_matched[i] = mtime_matches(...) (the
 * caller's tolerance rule), node_hashes[2i..2i+1] = node.hash() (lo, hi);
 * node_meta_present[i] / node_meta_hashes[2i..2i+1] = node.metadata_hash() (Some / its value; both
 * NULL: None for every item); file_meta_kind[i] (OXH_META_*; NULL: OXH_META_NONE for every item) says
 * how the working file's maybe_get_metadata_hash(get_file_metadata(path, data_type)) (fs.rs:1601-1607)
 * is obtained, with file_meta_hashes[2i..2i+1] its value for OXH_META_GIVEN. In the reference's order:
 *   sizes[i] != node_bytes[i]  -> modified[i] = 1, file not read                      (fs.rs:1590-1592)
 *   else mtime_matched[i]      -> modified[i] = 0, file not read                      (fs.rs:1595-1597)
 *   else OXH_META_ERROR        -> status[i] = OXH_ERR_META (the reference's `?`), file not read
 *   else node and file metadata hashes both Some and different -> modified[i] = 1     (fs.rs:1609-1614)
 *        (OXH_META_GIVEN: decided before any read; OXH_META_TEXT: MetadataText {num_lines, num_chars}
 *        is counted on the hashing read itself (K1T, repositories/metadata/text.rs:11-20) and its
 *        serde_json `{"text":{"num_lines":L,"num_chars":C}}` hashed on the device)
 *   else modified[i] = (get_hash_given_metadata(path) != node.hash())                (fs.rs:1616-1618)
 * Every file that has to be read is read once, all of them in one engine request (oxh_hash_files_meta
 * semantics, read to EOF). status[i] = OXH_OK, OXH_ERR_META as above, or the read error of a file
 * that had to be read (modified[i] = 0 then; the reference returns that error). status and n_hashed
 * (the count of files read) may be NULL. */
#define OXH_ERR_META 6      /* the caller's metadata extraction failed (per item, oxh_files_modified) */
#define OXH_META_NONE 0     /* the file's metadata hash is None (no metadata for its data type) */
#define OXH_META_GIVEN 1    /* the caller computed it: file_meta_hashes[2i..2i+1] */
#define OXH_META_TEXT 2     /* data type Text: counted on the hashing read and hashed on the device */
#define OXH_META_ERROR 3    /* the caller's extraction returned an error */
int oxh_files_modified(oxh_ctx* ctx, const char* const* paths, const uint64_t* sizes, const uint64_t* node_bytes,
                       const uint8_t* mtime_matched, const uint64_t* node_hashes, const uint8_t* node_meta_present,
                       const uint64_t* node_meta_hashes, const uint8_t* file_meta_kind, const uint64_t* file_meta_hashes,
                       uint64_t n, uint8_t* modified, int32_t* status, uint64_t* n_hashed);
/* oxh_files_modified plus os_error[i] (may be NULL) as in oxh_hash_files_ex for items whose read failed. */
int oxh_files_modified_ex(oxh_ctx* ctx, const char* const* paths, const uint64_t* sizes, const uint64_t* node_bytes,
                          const uint8_t* mtime_matched, const uint64_t* node_hashes, const uint8_t* node_meta_present,
                          const uint64_t* node_meta_hashes, const uint8_t* file_meta_kind, const uint64_t* file_meta_hashes,
                          uint64_t n, uint8_t* modified, int32_t* status, int32_t* os_error, uint64_t* n_hashed);
/* Device-resident is_utf8 sniff: d_flags[i] (int32) for item i of the arena (first 4 KiB). */
int oxh_utf8_prefix_device(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens, uint64_t n,
                           int32_t* d_flags, void* stream);
/* Device-resident K1T: as oxh_xxh3_128_batch_device plus d_counts (2n u64: num_lines, num_chars). */
int oxh_xxh3_128_text_batch_device(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens,
                                   uint64_t n, uint64_t* d_out, uint64_t* d_counts, void* stream);

/* ---------------------------------------------------------------- content-defined chunking
 * FastCDC v2020 as the block-level dedup experiment runs it (experiments/block-level-dedup/src/
 * chunker/fastcdchunker.rs:83-98: `v2020::FastCDC::new(&content, 4096, chunk, 2 * chunk)`, crate
 * fastcdc 3.2.1, Normalization::Level1, then `xxh3_128` of every chunk).
 *
 * Chunks n device-resident buffers (file i = d_arena[offsets[i] .. offsets[i] + lens[i]); `offsets`
 * and `lens` are HOST arrays). On return first_chunk[0..n] (host, n+1 entries) holds each file's
 * first chunk index; chunk k is d_arena[d_chunk_offsets[k] .. + d_chunk_lens[k]) (device arrays of
 * `capacity` entries; oxh_fastcdc_max_chunks gives a bound). If d_digests is not NULL it receives
 * XXH3-128 (lo, hi) of every chunk (2*capacity u64). Parameter ranges are the crate's asserts
 * (min 64..1 MiB, avg 256..4 MiB, max 1 KiB..16 MiB, level 0..3); out-of-range -> OXH_ERR_INVALID.
 * Blocks until the chunk table is complete. */
int oxh_fastcdc_device(const void* d_arena, const uint64_t* offsets, const uint64_t* lens, uint64_t n,
                       uint32_t min_size, uint32_t avg_size, uint32_t max_size, uint32_t level,
                       uint64_t* d_chunk_offsets, uint64_t* d_chunk_lens, uint64_t* d_digests, uint64_t capacity,
                       uint64_t* first_chunk, void* stream);
/* FastCDC from host memory to host memory: the block-level dedup chunker as the reference runs it --
 * fs::read(input_file), v2020 chunking, xxh3_128 per chunk (fastcdchunker.rs:75-98) -- over n files
 * (oxh_fastcdc_files: paths; each opened and read whole, its size from fstat) or n host buffers
 * (oxh_fastcdc_host). The bytes stream through a bounded pipeline: parallel reads into a pinned
 * bounce ring, H2D on a side stream into one of two device pieces of OXH_CDC_PIECE_MIB (default 1 GiB),
 * chunked by oxh_fastcdc_device while the next piece is read. A file larger than what is left of a
 * piece is chunked in segments; a chunk is kept only once `max_size` bytes after its start are known
 * and the next segment is chunked from the first one that was not (a cut depends only on its start
 * and the max bytes after it), so every boundary is the one the crate finds in the whole file.
 * Output, in host memory: chunk k = bytes [chunk_offsets[k], + chunk_lens[k]) of its file (the
 * crate's Chunk.offset / length), digests[2k..2k+1] its XXH3-128 (lo, hi; NULL = boundaries only);
 * file i's chunks are first_chunk[i] .. first_chunk[i+1]-1 (n+1 entries). A file that cannot be
 * opened (status OXH_ERR_OPEN) or read (OXH_ERR_IO, e.g. EISDIR, or the file ended early: os_error 0)
 * has no chunks; the others are unaffected. sizes / status / os_error may be NULL. More chunks than
 * `capacity` fail the call with OXH_ERR_INVALID (the text holds the count needed); the
 * oxh_fastcdc_max_chunks bound of the sizes always suffices. Parameter ranges as oxh_fastcdc_device. */
int oxh_fastcdc_files(oxh_ctx* ctx, const char* const* paths, uint64_t n, uint32_t min_size, uint32_t avg_size,
                      uint32_t max_size, uint32_t level, uint64_t* chunk_offsets, uint64_t* chunk_lens, uint64_t* digests,
                      uint64_t capacity, uint64_t* first_chunk, uint64_t* sizes, int32_t* status, int32_t* os_error);
int oxh_fastcdc_host(oxh_ctx* ctx, const uint8_t* const* bufs, const uint64_t* lens, uint64_t n, uint32_t min_size,
                     uint32_t avg_size, uint32_t max_size, uint32_t level, uint64_t* chunk_offsets, uint64_t* chunk_lens,
                     uint64_t* digests, uint64_t capacity, uint64_t* first_chunk);
/* Upper bound on the chunk count of files of these lengths (every chunk but a file's last is >= min). */
uint64_t oxh_fastcdc_max_chunks(const uint64_t* lens, uint64_t n, uint32_t min_size);
/* Fixed-size chunk digests from host memory to host memory: the block-level dedup's fixed-size
 * chunkers (fixedsize_multithreaded.rs:78-110 -- chunk i = [i*chunk_size, min((i+1)*chunk_size, size)),
 * xxh3_128 of each -- and fixedsize.rs:67-91, which reads the same chunks through a BufReader) over n
 * files (oxh_chunk_digests_files) or n host buffers (oxh_chunk_digests_host), through the same pipeline
 * as oxh_fastcdc_files (segments of whole chunks, so nothing is carried between them). File i's
 * chunks are first_chunk[i] .. first_chunk[i+1]-1 (n+1 entries), digests[2k..2k+1] = XXH3-128 (lo, hi)
 * of chunk k; an empty file has none. Errors per file as oxh_fastcdc_files. `capacity` entries of
 * `digests`; the count needed is sum(ceil(size_i / chunk_size)) (more fails with OXH_ERR_INVALID,
 * "need N entries"). chunk_size 0 -> OXH_ERR_INVALID ("Chunk size cannot be zero", fixedsize.rs:43-47);
 * chunk_size is at most 3 GiB - 64 MiB (a chunk fits one device piece). */
int oxh_chunk_digests_files(oxh_ctx* ctx, const char* const* paths, uint64_t n, uint64_t chunk_size, uint64_t* digests,
                            uint64_t capacity, uint64_t* first_chunk, uint64_t* sizes, int32_t* status, int32_t* os_error);
int oxh_chunk_digests_host(oxh_ctx* ctx, const uint8_t* const* bufs, const uint64_t* lens, uint64_t n,
                           uint64_t chunk_size, uint64_t* digests, uint64_t capacity, uint64_t* first_chunk);
/* oxh_fastcdc_files / oxh_chunk_digests_files over several contexts (one per device, so one PCIe link,
 * pipeline and reader pool each): the files split into nctx contiguous shares balanced by
 * their stat sizes, the shares run side by side, and the tables come back concatenated in file order --
 * every output exactly as the single-context call gives it. Contexts may repeat (shares on the same
 * context run one after the other). A failing share fails the call with its text ("share k ..."). */
int oxh_fastcdc_files_multi(oxh_ctx* const* ctxs, int nctx, const char* const* paths, uint64_t n, uint32_t min_size,
                            uint32_t avg_size, uint32_t max_size, uint32_t level, uint64_t* chunk_offsets,
                            uint64_t* chunk_lens, uint64_t* digests, uint64_t capacity, uint64_t* first_chunk,
                            uint64_t* sizes, int32_t* status, int32_t* os_error);
int oxh_chunk_digests_files_multi(oxh_ctx* const* ctxs, int nctx, const char* const* paths, uint64_t n,
                                  uint64_t chunk_size, uint64_t* digests, uint64_t capacity, uint64_t* first_chunk,
                                  uint64_t* sizes, int32_t* status, int32_t* os_error);
/* ... and the host-buffer entries (oxh_fastcdc_host / oxh_chunk_digests_host) the same way, the shares
 * balanced by the buffers' lengths. */
int oxh_fastcdc_host_multi(oxh_ctx* const* ctxs, int nctx, const uint8_t* const* bufs, const uint64_t* lens, uint64_t n,
                           uint32_t min_size, uint32_t avg_size, uint32_t max_size, uint32_t level, uint64_t* chunk_offsets,
                           uint64_t* chunk_lens, uint64_t* digests, uint64_t capacity, uint64_t* first_chunk);
int oxh_chunk_digests_host_multi(oxh_ctx* const* ctxs, int nctx, const uint8_t* const* bufs, const uint64_t* lens, uint64_t n,
                                 uint64_t chunk_size, uint64_t* digests, uint64_t capacity, uint64_t* first_chunk);
/* The compiled-in GEAR table (256 u64) and the (mask_s, mask_l) pair for an average size and
 * normalization level (fastcdc v2020 MASKS[bits +/- level], bits = round(log2(avg))). Host only. */
int oxh_fastcdc_gear(uint64_t* out256);
int oxh_fastcdc_masks(uint32_t avg_size, uint32_t level, uint64_t* mask_s, uint64_t* mask_l);

/* ---------------------------------------------------------------- dedup index
 * Which chunks are duplicates: the question the block-level dedup experiment answers through the file
 * system, one stat or file creation per chunk (fixedsize.rs:78-89 `chunk_path.exists()`,
 * fastcdchunker.rs:95-108 writes every chunk). The index is a hash table in device memory keyed by the
 * 128-bit chunk digests, persistent across calls. Every inserted row has an ORDINAL: the number of rows
 * inserted before its call plus its position in the call. For each row the index answers "which ordinal
 * first carried this digest" -- a row is a first occurrence exactly when that is its own ordinal.
 * The handle is opaque (like `stream`). The index uses `ctx`'s device and streams: destroy it before the
 * context. Calls on one index serialise on its mutex and ordinals follow lock order, so every result is
 * a pure function of the sequence of calls. The table grows as rows arrive (load kept at or below one
 * half; memory is 16 B per row of keys plus 16-32 B per row of table); when a larger table or key store
 * cannot be allocated the call returns OXH_ERR_NOMEM and the index is unchanged. n == 0 is OXH_OK and
 * touches nothing. Without a gfx950 device, create fails with OXH_ERR_NODEVICE. */
int oxh_dedup_index_create(oxh_ctx* ctx, uint64_t capacity_rows, void** out);   /* 0 = small default; grows */
int oxh_dedup_index_destroy(void* index);
/* Insert n digests (device: 2n u64, lo then hi; d_lens may be NULL). d_first (device, n u64, may be
 * NULL) = smallest ordinal carrying the same digest, over everything inserted so far including this
 * call. stats (host, 4 u64, may be NULL) = {new distinct rows, their bytes, duplicate rows, their bytes}.
 * Blocks until complete. */
int oxh_dedup_index_insert_device(void* index, const uint64_t* d_digests, const uint64_t* d_lens, uint64_t n,
                                  uint64_t* d_first, uint64_t* stats, void* stream);
int oxh_dedup_index_insert_host(void* index, const uint64_t* digests, const uint64_t* lens, uint64_t n,
                                uint64_t* first, uint64_t* stats);
/* Look up without inserting: first[i] = ordinal of the first row with that digest, or ~0 if absent. */
int oxh_dedup_index_query_device(void* index, const uint64_t* d_digests, uint64_t n, uint64_t* d_first, void* stream);
int oxh_dedup_index_query_host(void* index, const uint64_t* digests, uint64_t n, uint64_t* first);
/* out4 = {rows, distinct digests, bytes, distinct bytes} over the index's lifetime. */
int oxh_dedup_index_counts(void* index, uint64_t* out4);

/* ---------------------------------------------------------------- chunk overlap between file versions
 * How many chunks of one version of a file another version also holds: what the experiment's TestOxen
 * command asks of the n latest commits (chunker/oxendedup.rs:72-209, `OxenChunker::pack`), pair by pair
 * through `count_commit_overlap` (:56-70) -- for every hash of commit 1, with multiplicity, a
 * `Vec<String>::contains` scan of commit 2. Here all sets are counted against all in one call.
 * N = set_first[nsets] rows of (lo, hi) digests, set k = rows [set_first[k], set_first[k+1]); set_first
 * (nsets + 1 entries, set_first[0] = 0, non-decreasing), rows_out and bytes_out are HOST arrays in both
 * forms. rows_out[a * nsets + b] = the rows of set a, with multiplicity, whose digest occurs at least once
 * in set b: the diagonal is set a's row count, `count_commit_overlap(c1, c2)` is entry [c1][c2], and the
 * matrix is not symmetric when a set repeats a digest. bytes_out (may be NULL; needs the lengths) = the
 * same sum over the rows' lengths. Blocks until complete. The call keeps nothing: it builds a table of
 * its own on the device and frees it, and touches no oxh_dedup_index_* handle of the context.
 * OXH_ERR_INVALID: NULL set_first / rows_out, nsets 0 or above OXH_CHUNK_OVERLAP_MAX_SETS, a set_first
 * that does not start at 0 or decreases, N > 2^40, NULL digests with N > 0, bytes_out without lengths --
 * all before OXH_ERR_NODEVICE (there is no CPU path), then a NULL ctx. N == 0: OXH_OK, zeroed outputs.
 * A failed device allocation is OXH_ERR_NOMEM with the outputs untouched (memory: 40-56 B per row, 8 more
 * in the host form with lengths, plus 8 * ceil(nsets / 64) B per row of set masks). */
#define OXH_CHUNK_OVERLAP_MAX_SETS 256   /* TestOxen's n_commits is a u8 */
int oxh_chunk_overlap_device(oxh_ctx* ctx, const uint64_t* d_digests, const uint64_t* d_lens,
                             const uint64_t* set_first, uint64_t nsets, uint64_t* rows_out, uint64_t* bytes_out,
                             void* stream);
int oxh_chunk_overlap_host(oxh_ctx* ctx, const uint64_t* digests, const uint64_t* lens, const uint64_t* set_first,
                           uint64_t nsets, uint64_t* rows_out, uint64_t* bytes_out);

/* ---------------------------------------------------------------- row hashes of a data frame, and the row set-diff
 * `oxen diff` / `oxen df` on tabular files: core/df/tabular.rs:816-945 (`df_hash_rows`,
 * `df_hash_rows_on_cols`) hashes every row of a frame -- `any_val_to_bytes` (:651-675) of each cell appended
 * to one buffer, `hasher::hash_buffer` of it -- and repositories/diffs.rs:1023-1074
 * (`compute_new_row_indices`) builds two HashMap<String, u32> over the hex strings to say which rows were
 * added and which removed. Here the frame stays columnar (Arrow: values, offsets, validity bitmaps).
 *
 * A row's bytes are the concatenation, over the ncols columns IN THE ORDER GIVEN (the caller passes the
 * frame's schema order), of each cell's bytes: none for a null; the raw little-endian bytes of a
 * fixed-width cell (Int8: 1; Int32 / Float32: 4; Int64 / Float64 / Datetime(ms): 8); one byte 0 or 1 for a
 * boolean; the UTF-8 bytes of a string. Every other dtype goes through to_string() in the reference: the
 * caller renders such a column to strings and passes it as a byte column. Cells are not delimited, so
 * ("ab","c") and ("a","bc") collide, as in the reference; a row of all nulls hashes the empty input.
 * out[2r], out[2r+1] = XXH3-128 (lo, hi), seed 0, of row r's bytes.
 *
 * Columns are parallel arrays of ncols entries: kinds[c] (OXH_COL_*), values[c], offsets[c] (byte columns:
 * nrows + 1 int32 / int64, row r = values[c][offsets[c][r] .. offsets[c][r+1]); offsets[c][0] need not be
 * 0; ignored for the other kinds), validity[c] (NULL: no nulls; else an Arrow validity bitmap, row r's bit
 * being bit bit_offsets[2c+1] + r, LSB first) and bit_offsets[2c] (OXH_COL_BOOL: row r's value is bit
 * bit_offsets[2c] + r of values[c]). Bit offsets need not be multiples of 8 (a sliced Arrow array).
 * kinds, bit_offsets and the three pointer arrays are HOST arrays in both forms and none may be NULL; what
 * the pointers point to is on the device in _device (d_out too) and on the host in _host. Offsets must not
 * decrease or be negative: the host form checks them (OXH_ERR_INVALID) and copies only the span
 * [offsets[0], offsets[nrows]) of a byte column; the device form never reads outside the range a pair of
 * offsets names -- a bad pair is a cell of length 0, and the call returns OXH_ERR_INVALID. Both forms block
 * until complete.
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path): a NULL array, ncols == 0, an unknown
 * kind, more than 2^40 rows, then -- with rows -- NULL offsets of a byte column, NULL values (but for a byte
 * column whose span is empty; the device form learns that on the device), a NULL out; then a NULL ctx.
 * nrows == 0 (after the first four checks) is OXH_OK and touches nothing. A failed allocation is
 * OXH_ERR_NOMEM with the outputs untouched. */
#define OXH_COL_FIXED1 1      /* Int8 */
#define OXH_COL_FIXED4 4      /* Int32, Float32 */
#define OXH_COL_FIXED8 8      /* Int64, Float64, Datetime(ms) */
#define OXH_COL_BOOL 16       /* Arrow bit-packed booleans, LSB first */
#define OXH_COL_BYTES32 32    /* bytes + nrows+1 int32 offsets (Arrow Utf8/Binary) */
#define OXH_COL_BYTES64 64    /* bytes + nrows+1 int64 offsets (LargeUtf8/LargeBinary) */
int oxh_row_hashes_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                          const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                          uint64_t* d_out, void* stream);
int oxh_row_hashes_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* values,
                        const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets, uint64_t* out);
/* compute_new_row_indices over two digest tables (2 * n u64 each, (lo, hi) rows, as the row hashes above):
 * HashMap::from_iter keeps the LAST row index of each distinct hash; `added` is that index for every distinct
 * head digest absent from base, `removed` the mirror image. The device form writes one byte per row
 * (d_removed: nbase, d_added: nhead; 1 = reported) and counts2 (host) = {removed, added}; the host form
 * writes the ascending index lists (capacity nbase / nhead; u32, as the reference's Vec<u32>) and counts2.
 * Either side may have 0 rows (its table and output may then be NULL). Both block until complete and keep
 * nothing: a table of their own is built on the device and freed (memory: 56-72 B per row).
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE: NULL counts2, more than 2^32 - 1 rows on a side, a NULL table
 * or output of a side with rows; then a NULL ctx. No rows at all: OXH_OK, counts2 = {0, 0}. A failed
 * allocation is OXH_ERR_NOMEM with the outputs untouched. */
int oxh_row_diff_device(oxh_ctx* ctx, const uint64_t* d_base, uint64_t nbase, const uint64_t* d_head, uint64_t nhead,
                        uint8_t* d_removed, uint8_t* d_added, uint64_t* counts2, void* stream);
int oxh_row_diff_host(oxh_ctx* ctx, const uint64_t* base, uint64_t nbase, const uint64_t* head, uint64_t nhead,
                      uint32_t* removed_idx, uint32_t* added_idx, uint64_t* counts2);

/* ---------------------------------------------------------------- keyed tabular diff
 * `oxen diff --keys ... --targets ...` after the four df_hash_rows_on_cols passes (repositories/diffs.rs:
 * 881-901 `diff_dfs`, :1009-1021 `hash_dfs`): repositories/diffs/join_diff.rs full-joins the two frames on
 * the key hash (:290), labels every joined row through `test_function` (:458-484), filters the unchanged
 * ones out (:88-92), counts the rest (:434-456) and counts the rows of duplicated keys on each side
 * (core/df/tabular.rs:263-271 `n_duped_rows`). Here the join, the labels and the counts are one call over
 * the digest tables; nothing row-shaped crosses the link but the result.
 *
 * Per side (left = df_1, right = df_2): the key digests (2 * n u64 of (lo, hi) rows, as oxh_row_hashes_*
 * writes them), the target digests (the same shape; NULL = the reference's null column, no named target
 * is in that frame) and the validity bitmap of the cell of keys[0] -- the first key AS THE CALLER LISTED
 * IT -- (Arrow, LSB first, row r of the left side = bit bit_offsets2[0] + r, of the right side bit
 * bit_offsets2[1] + r; NULL = no nulls; offsets need not be multiples of 8). bit_offsets2 and counts8 are
 * HOST arrays in both forms; every other pointer is device memory in _device and host memory in _host.
 *
 * Joined rows: every (l, r) whose key digests are equal (the whole cross product when a key repeats),
 * (l, none) for a left row without a partner, (none, r) for a right row without one. Status, in the order
 * test_function tests: 1. left absent or the left row's keys[0] cell null -> ADDED (a matched pair too);
 * 2. else right absent or the right row's keys[0] cell null -> REMOVED; 3. else both target tables NULL ->
 * UNCHANGED; 4. else the target digests differ -> MODIFIED (NULL equals NULL and differs from every
 * digest, so with one table NULL every pair that gets here is MODIFIED); 5. else UNCHANGED.
 *
 * counts8 = {emitted pairs, added, removed, modified, unchanged, rows of duplicated keys left, right,
 * pairs written}; [1..4] count all joined rows whatever the flag. Emitted are all joined rows with
 * OXH_KEYED_DIFF_KEEP_UNCHANGED, the not-UNCHANGED ones without. The pairs go to three parallel arrays of
 * `capacity` entries, left_idx / right_idx (OXH_KEYED_DIFF_NONE = absent) and status (OXH_DIFF_*), ONLY
 * when emitted <= capacity (then counts8[7] == counts8[0]); otherwise counts8[7] = 0, the arrays are
 * untouched and the call is still OXH_OK: call again with counts8[0]. capacity == 0 with NULL arrays is
 * the counts-only call. nleft + nright entries are enough whenever no key repeats on the right.
 * Order of the pairs: the left rows ascending, each followed by its pairs or its one (l, none); then the
 * right-only rows ascending. Within one left row's pairs the host form writes the right rows ascending;
 * the DEVICE FORM MAY WRITE THEM IN ANY ORDER (only the rows of a key that repeats on the right are
 * affected), and that order may differ from call to call.
 *
 * Both forms block until complete and keep nothing: a private index and one device block are freed once
 * the stream has drained, and no oxh_dedup_index_* handle of the context is touched (memory: 68-84 B per
 * row of both sides together, 4 B more per right row; the host form adds the tables it copies, 16-32 B per
 * row, and 9 B per emitted pair).
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path): NULL counts8 or bit_offsets2; more than
 * 2^32 - 2 rows on a side; a NULL key table of a side with rows; a target table of a side with rows that
 * overlaps that side's key table without being the same pointer (two tables of n rows cannot share part
 * of their bytes; the same pointer -- keys and targets naming the same columns -- is fine); capacity > 0
 * with a NULL array; a flag bit other than OXH_KEYED_DIFF_KEEP_UNCHANGED; then a NULL ctx. No rows at
 * all: OXH_OK, counts8 zeroed. A failed allocation is OXH_ERR_NOMEM with the outputs untouched. */
#define OXH_KEYED_DIFF_KEEP_UNCHANGED 1
#define OXH_KEYED_DIFF_NONE 0xFFFFFFFF
#define OXH_DIFF_UNCHANGED 0
#define OXH_DIFF_ADDED 1
#define OXH_DIFF_REMOVED 2
#define OXH_DIFF_MODIFIED 3
int oxh_keyed_diff_device(oxh_ctx* ctx, const uint64_t* d_left_keys, uint64_t nleft, const uint64_t* d_right_keys,
                          uint64_t nright, const uint64_t* d_left_targets, const uint64_t* d_right_targets,
                          const uint8_t* d_left_key0_valid, const uint8_t* d_right_key0_valid, const uint64_t* bit_offsets2,
                          uint32_t flags, uint64_t capacity, uint32_t* d_left_idx, uint32_t* d_right_idx, uint8_t* d_status,
                          uint64_t* counts8, void* stream);
int oxh_keyed_diff_host(oxh_ctx* ctx, const uint64_t* left_keys, uint64_t nleft, const uint64_t* right_keys, uint64_t nright,
                        const uint64_t* left_targets, const uint64_t* right_targets, const uint8_t* left_key0_valid,
                        const uint8_t* right_key0_valid, const uint64_t* bit_offsets2, uint32_t flags, uint64_t capacity,
                        uint32_t* left_idx, uint32_t* right_idx, uint8_t* status, uint64_t* counts8);

/* ---------------------------------------------------------------- take: the columns of the joined rows
 * What join_diff.rs returns is the frame TabularDiff.contents: the key columns coalesced right-then-left
 * (:95-102), the targets' and display columns' `.left` / `.right` sides, the status. With the pairs of
 * oxh_keyed_diff_* on the device, those columns are one take (gather by row index) of the two frames'
 * Arrow columns, null indices included, with an optional fallback source (polars' `coalesce`).
 *
 * Sources: nsrc columns, described as oxh_row_hashes_* takes them (kinds, values, offsets, validity,
 * bit_offsets[2c] / [2c+1]), and src_rows[c], the rows of column c (the two frames differ in height).
 * Indices: idx0 and idx1, nout_rows u32 each -- the keyed diff's left_idx / right_idx as it writes them;
 * OXH_TAKE_NULL (the value of OXH_KEYED_DIFF_NONE) = absent; either may be NULL = all absent.
 * Outputs: nout columns, each four u32 at plan[4 * o]: the source column a, the index array a is read
 * through (0 or 1), a fallback source column b or OXH_TAKE_NO_COLUMN, the index array b is read through.
 * Cell (o, i) is the cell of column a at row idx[ia][i] if that index is present and the cell valid; else
 * the cell of column b at idx[ib][i] if b exists, that index is present and the cell valid; else null. The
 * output's kind is kinds[a]; kinds[b] must equal it. kinds, bit_offsets, src_rows, plan, value_capacity,
 * value_bytes, written and the six pointer arrays are HOST arrays in both forms; what the pointers (and
 * idx0 / idx1) point to is on the device in _device and on the host in _host.
 *
 * Output layout, fully defined (Arrow buffers that start at bit / offset 0): out_validity[o] is
 * ceil(nout_rows / 8) bytes, always written, pad bits 0. Fixed-width values: nout_rows * width bytes, a null
 * cell's value 0. Booleans: bit-packed, ceil(nout_rows / 8) bytes, null cells and pad bits 0. Byte columns:
 * nout_rows + 1 offsets of the column's own width (int32 / int64) from 0 in out_offsets[o] and the values
 * tightly packed; a null cell is an empty span. A BYTES32 output of more than 2^31 - 1 bytes is
 * OXH_ERR_INVALID (pass the column as BYTES64); nothing is written.
 *
 * Capacity (the keyed diff's contract): value_capacity[o] = the room of out_values[o] of a byte column (the
 * other kinds have the sizes above). value_bytes[o] = what column o's values need, filled on every successful
 * call. The outputs are written ONLY when every byte column fits, then *written = 1; otherwise *written = 0,
 * no output array is touched and the call is still OXH_OK: call again with value_bytes. out_values,
 * out_offsets and out_validity all NULL (value_capacity is then not read) is the sizes-only call.
 * The device form writes the bit-packed outputs (validity, boolean values) a 64-row word at a time: they
 * must be 8-byte aligned.
 *
 * Both forms block until complete and keep nothing. The host form copies to the device only what the rows
 * name (as oxh_row_hashes_host) and the two index arrays, runs the device path into a second block once the
 * sizes are known, and copies the outputs back.
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path): a NULL kinds, values, offsets, validity,
 * bit_offsets, src_rows or plan; nsrc == 0 or nout == 0; an unknown kind; a plan entry naming a column that
 * is not there or an index array above 1; kinds[a] != kinds[b]; nout_rows or a src_rows[c] above 2^32 - 2;
 * NULL value_bytes or written; a byte source column with rows and no offsets; in the host form, offsets that
 * are negative or decrease, bytes without values; a column with rows and no values; some but not all of the
 * three output arrays NULL, outputs without value_capacity, a NULL or (device form) misaligned output of a
 * column that needs it; then a NULL ctx. nout_rows == 0 is OXH_OK: sizes 0, and out_offsets[o] of a byte
 * column gets its single 0 when outputs are given. On the device an index that is neither absent nor below
 * src_rows (the cell is null; nothing is read through it) and a decreasing or negative pair of offsets (a
 * cell of length 0) make the call return OXH_ERR_INVALID. A failed allocation is OXH_ERR_NOMEM with the
 * outputs untouched. */
#define OXH_TAKE_NULL 0xFFFFFFFF
#define OXH_TAKE_NO_COLUMN 0xFFFFFFFF
int oxh_take_columns_device(oxh_ctx* ctx, uint32_t nsrc, const uint32_t* kinds, const void* const* d_values,
                            const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                            const uint64_t* src_rows, uint64_t nout_rows, const uint32_t* d_idx0, const uint32_t* d_idx1,
                            uint32_t nout, const uint32_t* plan, const uint64_t* value_capacity, void* const* d_out_values,
                            void* const* d_out_offsets, uint8_t* const* d_out_validity, uint64_t* value_bytes, uint32_t* written,
                            void* stream);
int oxh_take_columns_host(oxh_ctx* ctx, uint32_t nsrc, const uint32_t* kinds, const void* const* values,
                          const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                          const uint64_t* src_rows, uint64_t nout_rows, const uint32_t* idx0, const uint32_t* idx1, uint32_t nout,
                          const uint32_t* plan, const uint64_t* value_capacity, void* const* out_values, void* const* out_offsets,
                          uint8_t* const* out_validity, uint64_t* value_bytes, uint32_t* written);

/* ---------------------------------------------------------------- concat: row ranges of frames, one after the other
 * The first and the last steps of `oxen df`'s chain (core/df/tabular.rs:443-589 `transform_lazy` /
 * `transform_slice_lazy`): `--vstack` is polars' vertical concat of frames (:449-463), `--slice`, `--head`,
 * `--tail` (:571-636) and the page of every data-frame view (opts/df_opts.rs:62-72 `SliceRange::for_page`) are
 * one row range of one frame. Both are the same operation on Arrow columns: write the rows
 * [first, first + count) of one or more source frames, one after the other, as fresh buffers that start at
 * bit / offset 0. A contiguous range needs no gather by row index: this call copies.
 *
 * Sources: nparts parts of ncols columns each; kinds[c] (OXH_COL_*) is shared by all parts. Column c of part p
 * is entry p * ncols + c of values, offsets and validity, described as oxh_row_hashes_* takes a column, with
 * its bit offsets at bit_offsets[2 * (p * ncols + c)] (OXH_COL_BOOL values) and [.. + 1] (validity).
 * part_rows[p] is the height of part p; first[p] / count[p] are the rows taken from it; count NULL = whole
 * parts (first is then not read). Parts may alias each other: the same frame taken twice is legal. A NULL
 * validity = all rows valid. kinds, bit_offsets, part_rows, first, count, value_capacity, value_bytes, written
 * and the six pointer arrays are HOST arrays in both forms; what the pointers point to is on the device in
 * _device and on the host in _host.
 *
 * Output: ncols columns of N = sum(count) rows in the take's layout (Arrow buffers that start at bit / offset
 * 0): out_validity[c] is ceil(N / 8) bytes, always written, pad bits 0, a part without validity contributing
 * ones. Fixed-width values: N * width bytes. Booleans: ceil(N / 8) bytes, pad bits 0. Byte columns: N + 1
 * offsets of the column's own width from 0 in out_offsets[c]; the bytes [offsets[first], offsets[first + count])
 * of each part follow one another in out_values[c] with no gap, and the output offsets are the source offsets
 * rebased. Values are copied AS THEY ARE, under null cells too: a null cell keeps whatever value or span its
 * source had, as Arrow's own concat does; only validity and pad bits are normalised. This differs from
 * oxh_take_columns_*, which zeroes and empties null cells; sources in the take's canonical form (null cells 0
 * and empty) give canonical output, and every output of this library is canonical. A BYTES32 output of more
 * than 2^31 - 1 bytes is OXH_ERR_INVALID (pass the column as BYTES64); nothing is written.
 *
 * Capacity (the take's contract unchanged): value_capacity[c] = the room of out_values[c] of a byte column.
 * value_bytes[c] = what column c's values need, filled on every successful call. The outputs are written ONLY
 * when every byte column fits, then *written = 1; otherwise *written = 0, no output array is touched and the
 * call is still OXH_OK: call again with value_bytes. out_values, out_offsets and out_validity all NULL
 * (value_capacity is then not read) is the sizes-only call. The device form finds the byte totals from one
 * small read-back of offsets[first] and offsets[first + count] per part and byte column, and writes the
 * bit-packed outputs (validity, boolean values) a 64-row word at a time: they must be 8-byte aligned.
 *
 * Both forms block until complete and keep nothing; their tables live in the context's scratch, so a second
 * call allocates nothing in the device form. The host form reads the sizes from its own offsets, copies to
 * the device only the taken ranges (as oxh_row_hashes_host copies only what the rows name), runs the device
 * path into a second block and copies the outputs back.
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path), in this order: a NULL kinds, values,
 * offsets, validity, bit_offsets or part_rows, or a NULL first with a count; nparts == 0 or ncols == 0; nparts
 * above OXH_CONCAT_MAX_PARTS; an unknown kind; first[p] + count[p] > part_rows[p]; a part_rows[p] or N above
 * 2^32 - 2; NULL value_bytes or written; a byte column with rows taken and no offsets; a column of another
 * kind with rows taken and no values; some but not all of the three output arrays NULL, outputs without
 * value_capacity, a NULL or (device form) misaligned output of a column that needs it; in the host form,
 * offsets that are negative or decrease inside a taken range, bytes without values; then a NULL ctx. N == 0 is
 * OXH_OK: sizes 0, and out_offsets[c] of a byte column gets its single 0 when outputs are given.
 * In the device form a byte column whose taken range holds bytes but that has no values is OXH_ERR_INVALID
 * after the read-back, nothing written. A negative or decreasing pair of offsets inside a taken range is
 * treated as in the other device forms -- nothing outside [offsets[first], offsets[first + count]) is read, and
 * nothing at all of a part whose span is itself negative or decreasing (its cells all have length 0); inside
 * a good span the offset AFTER a bad pair is written as the rebased offset before it, so that cell has length
 * 0, and every rebased offset is clamped into the part's span -- the call finishes, fills value_bytes and
 * written, and returns OXH_ERR_INVALID. A failed allocation is OXH_ERR_NOMEM with the outputs untouched. */
#define OXH_CONCAT_MAX_PARTS 65536
int oxh_concat_columns_device(oxh_ctx* ctx, uint32_t nparts, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                              const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                              const uint64_t* part_rows, const uint64_t* first, const uint64_t* count, const uint64_t* value_capacity,
                              void* const* d_out_values, void* const* d_out_offsets, uint8_t* const* d_out_validity,
                              uint64_t* value_bytes, uint32_t* written, void* stream);
int oxh_concat_columns_host(oxh_ctx* ctx, uint32_t nparts, uint32_t ncols, const uint32_t* kinds, const void* const* values,
                            const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                            const uint64_t* part_rows, const uint64_t* first, const uint64_t* count, const uint64_t* value_capacity,
                            void* const* out_values, void* const* out_offsets, uint8_t* const* out_validity, uint64_t* value_bytes,
                            uint32_t* written);

/* ---------------------------------------------------------------- stable multi-column row sort
 * join_diff.rs:107 sorts the joined frame with `sort_df_on_keys` (:146-163) before it selects the output
 * columns, and `oxen df --sort` (core/df/tabular.rs:520-522) sorts a frame on one column. Here the sort is a
 * device-wide stable radix sort over the key columns; its result is a permutation, directly usable as idx0
 * of oxh_take_columns_*.
 *
 * The order. It restates polars' documented defaults (`SortMultipleOptions::new().with_order_descending(false)`:
 * ascending, nulls_last = false); it is NOT pinned by a run of polars. Rows are compared key column by key
 * column, in the order the caller lists the keys. Within one column: a null comes before every value;
 * OXH_SORT_SIGNED: two's complement of the column's width (Int8, Int32, Int64, Datetime(ms));
 * OXH_SORT_UNSIGNED: plain unsigned of the column's width; OXH_SORT_FLOAT (widths 4 and 8 only): numeric
 * order, -0.0 equals +0.0, every NaN -- whatever its sign or payload -- equals every other NaN and is greater
 * than +inf; OXH_COL_BOOL: false before true (the order class is ignored); byte columns: unsigned byte-wise
 * lexicographic order, a proper prefix first, so "" < "a" < "a\0" < "a\0\0" < "b" and a null comes before ""
 * (the order class is ignored). Rows equal on every key keep their input order: the sort is STABLE. The
 * reference's sort is unstable; the stable result is one of those it may produce, and it is unique.
 * (`sort_df_on_keys` sorts on the keys that are `is_primitive()`, restated from memory as numeric | Boolean |
 * String | Binary: every kind a column here can have, so every key takes part. Unpinned as well.)
 *
 * Key columns are described exactly as oxh_row_hashes_* takes them (kinds, values, offsets, validity,
 * bit_offsets[2c] / [2c+1]); orders[c] is one of the three classes. kinds, bit_offsets, orders, stats3 and
 * the three pointer arrays are HOST arrays in both forms; what the pointers point to, and perm, is on the
 * device in _device and on the host in _host. perm[i] (nrows u32) = the input row that stands at place i of
 * the sorted frame. stats3 = {refinement rounds run, radix passes launched, rows that equal another row on
 * every key}. Both forms block until complete and keep nothing (memory: 86 B per row on the device, leased
 * for the call; the host form adds the key columns it copies and 4 B per row).
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path): a NULL kinds, values, offsets, validity,
 * bit_offsets or orders; nkeys == 0; an unknown kind, or an unknown order class of a fixed-width column;
 * OXH_SORT_FLOAT on a width-1 column; more than 2^32 - 2 rows; with rows: NULL offsets of a byte column, NULL
 * values (but for a byte column whose span is empty; the device form learns that on the device), a NULL perm;
 * NULL stats3; then a NULL ctx. nrows == 0 after the checks is OXH_OK: stats3 is zeroed, nothing else is
 * touched. A failed allocation is OXH_ERR_NOMEM with perm untouched. Offsets must not decrease or be
 * negative: the host form checks them; the device form treats a bad pair as a cell of length 0 and returns
 * OXH_ERR_INVALID. Neither form ever reads outside a named span. */
#define OXH_SORT_SIGNED 0
#define OXH_SORT_UNSIGNED 1
#define OXH_SORT_FLOAT 2
int oxh_sort_rows_device(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* d_values,
                         const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                         const uint32_t* orders, uint32_t* d_perm, uint64_t* stats3, void* stream);
int oxh_sort_rows_host(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* values,
                       const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                       const uint32_t* orders, uint32_t* perm, uint64_t* stats3);

/* ---------------------------------------------------------------- rows grouped by equality: unique, unique_count, duplicates
 * `oxen df --unique cols` (core/df/tabular.rs:424-427 `unique_df`: `df.unique(Some(columns),
 * UniqueKeepStrategy::First)`), `--unique_count cols` (:429-433 `unique_count_df`: `group_by(cols).agg([len()])`)
 * and `n_duped_rows` (:263-271: `select(cols).is_duplicated().sum()`) are three readings of one grouping of the
 * rows by equality on the key columns. Here that grouping is one call on the device; with oxh_sort_rows_* and
 * oxh_take_columns_* a caller replays `--unique label --sort image` without a host hash map in between.
 *
 * Equality. It restates polars' documented behaviour for `unique` / `group_by`; it is NOT pinned by a run of
 * polars. Rows are equal when they are equal in every key column. Within a column a null equals a null and
 * nothing else; fixed-width cells are equal when their bytes are, but under OXH_SORT_FLOAT (widths 4 and 8),
 * where -0.0 equals +0.0 and every NaN equals every NaN whatever its sign or payload -- the canonical form
 * the sort above orders by, from the same code; booleans are equal by value; byte cells when they have the same
 * length and the same bytes ("" is not null). Equality is decided on a 128-bit digest (XXH3-128) of an
 * injective image of the row's key -- every cell tagged null / present, a byte cell behind its length -- as
 * everywhere in this library; the undelimited row bytes of oxh_row_hashes_* cannot serve (("ab","c") and
 * ("a","bc"), (null, 5) and (5, null), null and "" collide there, as in the reference's diff).
 *
 * Key columns are described exactly as oxh_sort_rows_* takes them (kinds, values, offsets, validity,
 * bit_offsets[2c] / [2c+1], orders[c] one of OXH_SORT_*: only OXH_SORT_FLOAT changes equality, but the array is
 * taken and validated as the sort does, so a frame's sort plan is reusable as it is). kinds, bit_offsets, orders,
 * stats4 and the three pointer arrays are HOST arrays in both forms; what the pointers point to, and the four
 * outputs, are on the device in _device and on the host in _host. Outputs, u32 each, every one of them may be
 * NULL on its own (it is then not written):
 *   group[i]       (nrows) the smallest row whose key equals row i's: group[i] <= i, group[group[i]] == group[i];
 *   count[i]       (nrows) the rows of row i's group;
 *   first_idx[g], first_count[g]   for g < groups: the rows with group[i] == i, ascending, and their groups'
 *                  sizes. The caller provides nrows entries each; entries from `groups` on are untouched.
 *                  first_idx is the selection of unique(keep = First) with the first occurrences in input order
 *                  (polars' maintain_order form; the reference's order is unspecified and its tests sort
 *                  afterwards: this order is one it may produce, and it is unique), usable as idx0 of
 *                  oxh_take_columns_*.
 * stats4 (host, required) = {groups, rows whose group has two or more rows (is_duplicated().sum(), n_duped_rows),
 * the largest group, rows whose key image went through the long path (above 240 encoded bytes)}.
 * Both forms block until complete and keep nothing: a private index and a lease of device scratch end with the
 * call, and no oxh_dedup_index_* handle of the context is touched (memory: 40 B per row leased, plus the index's
 * 32-48 B per row: 72-88 B per row, and the images of the long rows; the host form adds the key columns it
 * copies and 16 B per row).
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path): the sort's list in the sort's order -- a NULL
 * kinds, values, offsets, validity, bit_offsets or orders; nkeys == 0; an unknown kind, or an unknown order class
 * of a fixed-width column; OXH_SORT_FLOAT on a width-1 column; more than 2^32 - 2 rows; with rows: NULL offsets of
 * a byte column, NULL values (but for a byte column whose span is empty; the device form learns that on the
 * device) -- then NULL stats4; then a NULL ctx. nrows == 0 after the checks is OXH_OK: stats4 is zeroed, nothing
 * else is touched. A failed allocation is OXH_ERR_NOMEM with the outputs untouched. Offsets must not decrease or
 * be negative: the host form checks them (nothing is written); the device form treats a bad pair as a cell of
 * length 0, finishes -- the outputs and stats4 are those of the frame with that cell empty -- and returns
 * OXH_ERR_INVALID. Neither form ever reads outside a named span. An id from the index that is not a row at or
 * before its own is never used as an index: the call returns OXH_ERR_HIP. */
int oxh_group_rows_device(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* d_values,
                          const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                          const uint32_t* orders, uint32_t* d_group, uint32_t* d_count, uint32_t* d_first_idx,
                          uint32_t* d_first_count, uint64_t* stats4, void* stream);
int oxh_group_rows_host(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* values,
                        const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                        const uint32_t* orders, uint32_t* group, uint32_t* count, uint32_t* first_idx, uint32_t* first_count,
                        uint64_t* stats4);

/* ---------------------------------------------------------------- row filter: `oxen df --filter` as selection indices
 * `oxen df --filter "label == dog && min_x > 0.5"` (core/df/tabular.rs:404-422 `filter_df`, :391-402
 * `filter_from_val`, the parser in core/df/filter.rs, the literal typing of :332-361 `val_from_str_and_dtype`)
 * is the step of `transform_lazy` in front of `unique`, `unique_count` and `sort`. Here it is one call on the
 * device whose result is the ascending array of the selected rows, directly usable as idx0 of
 * oxh_take_columns_*, and / or an Arrow bitmap of them.
 *
 * A filter is nterms terms `column OP literal`, OP one of == != < <= > >=, joined by nterms - 1 logical operators
 * && / ||. The operators are FOLDED LEFT TO RIGHT WITH NO PRECEDENCE: `a || b && c` is `(a || b) && c`, which is
 * what `filter_df` builds (`expr = expr.and(chain)` / `expr.or(chain)` in a loop).
 *
 * Semantics. They restate polars' documented behaviour; they are NOT pinned by a run of polars.
 *   Null cells: a term on a null cell is null, for every operator, != included (polars' `neq`, not `neq_missing`).
 *   Three-valued logic: && and || are Kleene's -- null && false = false, null || true = true, otherwise a null is
 *     contagious. A row is selected exactly when the folded result is TRUE; null and false rows are dropped.
 *   Fixed-width columns compare by the canonical word of the cell (the sort's and the grouping's, from the same
 *     code) against the same word of the literal: signed or unsigned by the column's order class;
 *     OXH_SORT_FLOAT in numeric order with -0.0 == +0.0, every NaN equal to every NaN and greater than +inf
 *     (polars' total-order comparisons).
 *   Booleans compare false < true.
 *   Byte columns compare unsigned byte-wise lexicographically, a proper prefix first; "" is a value, not null.
 *   Literals are typed by the column, as `val_from_str_and_dtype` does. The reference panics on Int8 / Int16 /
 *     UInt* columns (in `lit_from_any`), on Datetime, and on an unknown field; this library accepts every kind
 *     and order class a column can have, and returns an error where the reference would panic on an unknown
 *     field or an unparsable literal (the typing itself is the caller's: oxen_amd.tabular.filter_terms).
 *
 * Columns are described exactly as oxh_sort_rows_* takes them (ncols of them: kinds, values, offsets, validity,
 * bit_offsets[2c] / [2c+1], orders[c]) and validated by the same rules in the same order; only the columns a
 * term names are read. HOST arrays in both forms, beside those: term_col[t] (an index below ncols), term_op[t]
 * (OXH_FILTER_EQ ..), term_word[t] (the literal of a fixed-width term: its little-endian bytes, zero-extended;
 * of a boolean term: 0 / 1; unused for a byte term), lit_bytes and lit_offsets (nterms + 1 entries: a byte
 * term's literal is lit_bytes[lit_offsets[t] .. lit_offsets[t+1]); a term of another kind has an empty span),
 * logical (nterms - 1 entries of OXH_FILTER_AND / OXH_FILTER_OR; may be NULL when nterms == 1) and stats2.
 * What the column pointers point to, idx and mask are on the device in _device and on the host in _host.
 * Outputs, every one of which may be NULL but stats2:
 *   idx    u32: the selected rows, ascending. The caller provides nrows entries; entries from `selected` on are
 *          untouched. Usable as idx0 of oxh_take_columns_*.
 *   mask   8 * ceil(nrows / 64) bytes, 8-byte aligned: an Arrow bitmap, LSB first, bit i = row i is selected;
 *          the bits past nrows are zero. Usable as the values of a boolean column.
 *   stats2 (host, required) = {selected rows, rows whose folded result is null}.
 * Both forms block until complete and keep nothing (memory, leased for the call: 4.6 KiB of control words and
 * literals; with idx 12 B per 64 rows -- the selected rows of every 64-row block and their scan -- plus 8 B per 64
 * rows where mask is NULL: under 0.32 B per row; the host form adds the columns the terms name, as it copies them,
 * 4 B per row of idx and the mask).
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path), in this order: the sort's list in the sort's
 * order over the ncols columns (a NULL kinds, values, offsets, validity, bit_offsets or orders; ncols == 0; an
 * unknown kind, or an unknown order class of a fixed-width column; OXH_SORT_FLOAT on a width-1 column; more than
 * 2^32 - 2 rows; with rows: NULL offsets of a byte column, NULL values -- but for a byte column whose span is
 * empty; the device form learns that on the device); nterms == 0 or above OXH_FILTER_MAX_TERMS; a NULL term_col,
 * term_op, term_word or lit_offsets, or a NULL logical with nterms > 1; a term_col not below ncols; an unknown
 * operator or logical operator; a term_word above 1 for a boolean column; lit_offsets that decrease or pass
 * OXH_FILTER_MAX_LITERAL_BYTES; NULL lit_bytes with a non-empty literal; NULL stats2; then a NULL ctx.
 * nrows == 0 after the checks is OXH_OK: stats2 is zeroed, nothing else is touched. A failed allocation is
 * OXH_ERR_NOMEM with the outputs untouched. Offsets must not decrease or be negative: the host form checks them
 * (nothing is written); the device form treats a bad pair as a cell of length 0 (an empty byte cell, not a null),
 * finishes -- the outputs and stats2 are those of the frame with that cell empty -- and returns
 * OXH_ERR_INVALID. Neither form ever reads outside a named span. A place from the scan is checked against the
 * selected rows and the row before it is stored through; a bad one makes the call return OXH_ERR_HIP. */
#define OXH_FILTER_EQ 0
#define OXH_FILTER_NE 1
#define OXH_FILTER_LT 2
#define OXH_FILTER_LE 3
#define OXH_FILTER_GT 4
#define OXH_FILTER_GE 5
#define OXH_FILTER_AND 0
#define OXH_FILTER_OR 1
#define OXH_FILTER_MAX_TERMS 16
#define OXH_FILTER_MAX_LITERAL_BYTES 4096   /* all byte literals of one call together */
int oxh_filter_rows_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                           const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                           const uint32_t* orders, uint32_t nterms, const uint32_t* term_col, const uint32_t* term_op,
                           const uint64_t* term_word, const uint8_t* lit_bytes, const uint64_t* lit_offsets,
                           const uint32_t* logical, uint32_t* d_idx, uint64_t* d_mask, uint64_t* stats2, void* stream);
int oxh_filter_rows_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* values,
                         const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                         const uint32_t* orders, uint32_t nterms, const uint32_t* term_col, const uint32_t* term_op,
                         const uint64_t* term_word, const uint8_t* lit_bytes, const uint64_t* lit_offsets,
                         const uint32_t* logical, uint32_t* idx, uint64_t* mask, uint64_t* stats2);

/* ---------------------------------------------------------------- embedding similarity: mean query, cosine, ranked rows
 * `oxen df --find-embedding-where "id = 42" --sort-by-similarity-to embedding` and the server's nearest-neighbour
 * endpoint (repositories/workspaces/data_frames/embeddings.rs: `embedding_from_query` :297-328 selects the rows of
 * a WHERE clause and `get_avg_embedding` :569-641 averages their vectors; `build_similarity_query_sql` :331-358
 * computes `array_cosine_similarity(column, query::FLOAT[d])` for every row and orders by it DESC; `query` /
 * `nearest_neighbors` :413-567 cut one page out with LIMIT / OFFSET). The reference does this in DuckDB on the
 * CPU. Here the three steps are three calls on the device, and each takes or returns what its neighbours do:
 * the mean takes the idx of oxh_filter_rows_*, the similarity returns a permutation, the take gathers the page's
 * own embedding column by the same u32 indices as oxh_take_columns_*.
 *
 * The column. nrows vectors of exactly dim float32 values (dim >= 1), in one of three layouts:
 *   OXH_EMB_FIXED    Arrow FixedSizeList<float32>[dim]: row r's floats start at values + r * dim; offsets is not read;
 *   OXH_EMB_LIST32 / OXH_EMB_LIST64   Arrow List / LargeList of float32: nrows + 1 int32 / int64 offsets that count
 *                    ELEMENTS of values.
 * validity (may be NULL) is an Arrow bitmap whose bit validity_bit is row 0's; a null row is a null vector.
 * values needs 4-byte alignment only: a sliced array or an odd dim puts rows at any multiple of 4 bytes, and
 * every row is read correctly at any of them (4-byte loads up to the row's first 16-byte boundary, 16-byte loads
 * from there). Float64 lists and null ELEMENTS inside a vector are not representable here (`get_avg_embedding`
 * rejects the first with ExpectedF32, DuckDB's array functions error on the second): the caller refuses them.
 * In a list layout a VALID row whose length is not dim is never read; the call finishes, stats4 says how many
 * such rows there are and which is the first, and the call returns OXH_ERR_INVALID (the reference's
 * EmbeddingLengthMismatch). A null row's offsets are not looked at. No read ever goes through a decreasing or
 * negative pair of offsets or past a row's own span: the host forms check the offsets before anything is copied
 * (nothing is written), the device forms skip such a row, finish and return OXH_ERR_INVALID.
 *
 * Every entry takes the column as (layout, nrows, dim, values, offsets, validity, validity_bit); stats4 is a HOST
 * array in both forms; everything else a pointer names is on the device in _device and on the host in _host.
 * stats4 = {rows used (valid and of length dim), null rows, valid rows of another length, the smallest such row
 * -- nrows when there is none}, counted over the rows the call names. All forms block until complete and keep
 * nothing; their scratch is leased for the call. A host form copies to one device block only the span its rows
 * name (a list column: the elements [offsets[first], offsets[last + 1])), at the caller's phase within 16 bytes,
 * and leaves the caller's output arrays untouched unless it returns OXH_OK.
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path), in this order: an unknown layout; dim == 0;
 * more than 2^32 - 2 rows; with rows: values not 4-byte aligned, NULL values (in the host form of a list column:
 * only when its span is not empty), NULL offsets of a list column, in the host form offsets that are negative or
 * decrease; then the entry's own arguments (below); NULL stats4; in the host form an index that is not a row;
 * then a NULL ctx. nrows == 0 (the take: nout == 0) after the checks is OXH_OK: stats4 is zeroed, nothing else
 * is touched. A failed allocation is OXH_ERR_NOMEM with the outputs untouched.
 *
 * oxh_embedding_mean_*: out[d] (dim floats) = the mean of element d over the rows idx[0 .. nidx) -- ascending u32
 * row indices, exactly what oxh_filter_rows_* writes; on the device in _device. Null rows among them are skipped
 * and counted. With no row used out is untouched and the call is still OXH_OK (the caller says "no rows
 * found"). An index >= nrows is OXH_ERR_INVALID and that row is never read. Arithmetic: float32 sums, then one
 * division by the count as float32; no floating-point atomics. The rows are partitioned by nidx alone -- chunks
 * of 64 idx entries dealt round-robin to min(ceil(nidx / 64), 1024) workgroups, whose partial sums a second
 * kernel adds in workgroup order -- so the result is bit-identical from run to run and between the two forms.
 * Own arguments: more than 2^32 - 2 indices; with rows and indices a NULL idx or out.
 * The reference pushes only `array.value(0)` of every record batch, so with one batch it uses the first matching
 * row alone; here the mean is over ALL matching rows, which is what its comment and its name say. The two
 * agree where the clause matches one row.
 *
 * oxh_embedding_similarity_*: for every row the cosine similarity with `query` (dim floats; on the device in
 * _device). The semantics restate DuckDB's `array_cosine_similarity` and `ORDER BY .. DESC` from memory; they
 * are NOT pinned by a run of DuckDB:
 *   dot = sum x*q, nx = sum x*x, nq = sum q*q, each summed in float32 in an unspecified order;
 *   sim = dot / sqrtf(nx * nq) with IEEE divide and square root, then clamped to [-1, 1] by comparisons that let a
 *   NaN through: a zero row or a zero query gives NaN, NaN and inf elements propagate as IEEE says;
 *   a null row (and a row that is not read, above) gives a null similarity: validity bit 0, sim 0.0f.
 * Outputs: sim (nrows float32); sim_validity (ceil(nrows / 8) bytes, an Arrow bitmap from bit 0, the bits past
 * nrows zero; may be NULL when the column has no validity, and is all ones when given then); order_key (nrows
 * u32, may be NULL); perm (nrows u32, may be NULL, needs order_key).
 *   order_key is the DESCENDING order as an ascending unsigned key: for a valid row the bitwise NOT of the row
 *   sort's float32 word of sim (OXH_SORT_FLOAT, the same code), for a null row 0xFFFFFFFF. Ascending on it: NaNs
 *   first (DuckDB ranks NaN above every number), then +1 .. -1 with -0.0 equal to +0.0, then the nulls (DuckDB's
 *   default NULLS LAST). The largest valid key is 0xFF800000 (-inf): no valid key equals the null key.
 *   perm is the STABLE ascending sort of order_key -- equal similarities keep input order -- by oxh_sort_rows_device
 *   over that one OXH_COL_FIXED4 / OXH_SORT_UNSIGNED column; perm[i] = the row at place i, usable as idx0 of
 *   oxh_take_columns_* and as idx of oxh_embedding_take_*. In the device form perm is written even when the call
 *   returns OXH_ERR_INVALID for rows of another length (they rank as nulls).
 * Own arguments: perm without order_key; with rows a NULL query or sim, a column with validity and a NULL
 * sim_validity.
 *
 * oxh_embedding_take_*: the page's own embedding column. idx: nout u32 row indices, OXH_TAKE_NULL = absent. The
 * output is always in the fixed layout: out_values nout * dim floats, out_validity ceil(nout / 8) bytes from bit
 * 0 with the bits past nout zero, always written. An absent index, a null source row and a row that is not read
 * give dim zeros and validity bit 0 (stats4 counts all three as null rows but the last). An index that is neither
 * absent nor below nrows is OXH_ERR_INVALID; nothing is read through it.
 * Own arguments: more than 2^32 - 2 output rows; with output rows a NULL idx, out_values or out_validity. */
#define OXH_EMB_FIXED 0
#define OXH_EMB_LIST32 1
#define OXH_EMB_LIST64 2
int oxh_embedding_mean_device(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* d_values, const void* d_offsets,
                              const uint8_t* d_validity, uint64_t validity_bit, const uint32_t* d_idx, uint64_t nidx, void* d_out,
                              uint64_t* stats4, void* stream);
int oxh_embedding_mean_host(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* values, const void* offsets,
                            const uint8_t* validity, uint64_t validity_bit, const uint32_t* idx, uint64_t nidx, void* out,
                            uint64_t* stats4);
int oxh_embedding_similarity_device(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* d_values, const void* d_offsets,
                                    const uint8_t* d_validity, uint64_t validity_bit, const void* d_query, void* d_sim,
                                    uint8_t* d_sim_validity, uint32_t* d_order_key, uint32_t* d_perm, uint64_t* stats4, void* stream);
int oxh_embedding_similarity_host(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* values, const void* offsets,
                                  const uint8_t* validity, uint64_t validity_bit, const void* query, void* sim, uint8_t* sim_validity,
                                  uint32_t* order_key, uint32_t* perm, uint64_t* stats4);
int oxh_embedding_take_device(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* d_values, const void* d_offsets,
                              const uint8_t* d_validity, uint64_t validity_bit, const uint32_t* d_idx, uint64_t nout, void* d_out_values,
                              uint8_t* d_out_validity, uint64_t* stats4, void* stream);
int oxh_embedding_take_host(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* values, const void* offsets,
                            const uint8_t* validity, uint64_t validity_bit, const uint32_t* idx, uint64_t nout, void* out_values,
                            uint8_t* out_validity, uint64_t* stats4);

/* ---------------------------------------------------------------- CSV: record index and typed Arrow columns
 * `oxen df data.csv ..` and `oxen diff a.csv b.csv` first read the file (core/df/tabular.rs:39-71 read_df_csv,
 * base_lazy_csv_reader), and the tabular metadata reads it again for width, height and schema
 * (repositories/metadata/tabular.rs:10-25). oxh_csv_* do that on the device: CSV bytes in HBM to a record index (a
 * handle), then to columns in this header's own description (OXH_COL_*: values, offsets, validity) that every
 * tabular entry above takes as they are.
 *
 * The rules restate polars' documented reader under the reference's settings (header row, eol_char '\n',
 * truncate_ragged_lines, ignore_errors, a one-byte separator, an optional one-byte quote). They are NOT pinned by
 * a run of polars.
 *   Quotes by parity. With a quote byte configured, EVERY occurrence of it toggles "inside quotes", wherever it
 *     stands; a doubled quote toggles twice and changes nothing. On well-formed input this is RFC 4180; on
 *     malformed input (a stray quote in the middle of a field) it is not. With OXH_CSV_NO_QUOTE no byte is special.
 *   Records. A record ends at '\n' outside quotes. The end of the buffer ends the last record whatever the parity
 *     (stats8[7] says that the buffer ended inside quotes). One '\r' directly before the ending '\n' (or before the
 *     end of the buffer) is not part of the record's last field. A record of zero bytes, or of that one '\r', is
 *     skipped and counted.
 *   Fields. A record splits at the separators outside quotes.
 *   Field values. A field whose first and last bytes are both the quote (length >= 2) loses them, and every
 *     doubled quote inside becomes one (left to right: a run of k quotes keeps k - k / 2). Any other field is its
 *     bytes as they are.
 *   Header. With OXH_CSV_HAS_HEADER the first kept record is the header and its field count is ncols. Without it
 *     ncols is the first kept record's field count and that record is data.
 *   Ragged records. A short data record has nulls for its missing fields, a long one loses its extra fields (and
 *     the '\r' rule applies to the record's own last field only). Both are counted.
 *   Nulls. An empty unquoted field is null in every type. "" (quoted, empty) is an empty string in a string column
 *     and null in the others (counted with the empty fields).
 *   Types (grammars over the whole field value; no whitespace trimming):
 *     OXH_CSV_INT64    [+-]?[0-9]+ , exact; out of range is null, never wrapped;
 *     OXH_CSV_FLOAT64  [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?  or  [+-]?(inf|infinity|nan), ASCII
 *                      case-insensitive: the CORRECTLY ROUNDED double, bit for bit what C's strtod gives; NaN is
 *                      the quiet NaN 0x7FF8000000000000 with the sign as written;
 *     OXH_CSV_BOOL     true / false, ASCII case-insensitive;
 *     OXH_CSV_STRING / OXH_CSV_STRING64   the field value, with int32 / int64 offsets (OXH_COL_BYTES32 / 64).
 *     Text that does not match its grammar is null (ignore_errors), counted apart from the empty-field nulls. A
 *     null cell's value is 0 / false / no bytes.
 *   Floats. The device converts a cell itself where one IEEE operation is exact: at most 19 significant digits, a
 *     mantissa <= 2^53 and a decimal exponent within +-22 (double(m) * 10^e or double(m) / 10^-e, plain * and /),
 *     and the zeros, infinities and NaNs. Every other matching cell is DEFERRED: compacted on the device, its text
 *     brought down, converted on the host (std::from_chars; strtod in the "C" locale outside the doubles' range)
 *     and scattered back inside the same blocking call. stats4[2] counts them.
 *   Inference. Over the first max_rows data rows, per column the AND of each cell's class bits -- the value is an
 *     in-range INT64 / matches the FLOAT64 grammar / is a BOOL; an empty value (quoted or not) and a missing field
 *     have all three. Int64 if every cell is an integer, else Float64, else Boolean, else String; a column with
 *     every bit after no rows or only empty cells is String (OXH_CSV_STRING; the caller picks STRING64).
 *   Out of scope: dialect sniffing (qsv_sniffer: the caller passes separator and quote); the LossyUtf8
 *     replacement of invalid sequences (bytes are copied as they are); comment lines, skip_rows, multi-byte
 *     separators, dates; buffers of 2^32 bytes and more (OXH_ERR_INVALID: positions are u32); files larger than one
 *     device buffer (no piece pipeline).
 *
 * The handle (a void*, as the dedup index's) holds the index: `ends`, the u32 position of every separator and
 * record end outside quotes in ascending order (4 B per delimiter); `rec_end`, for every record the place of its
 * end in `ends` (4 B per record); `row_rec`, the kept records (4 B per record); and the header's names. Field f of
 * record r is the bytes between ends[first(r) + f - 1] + 1 and ends[first(r) + f], present iff first(r) + f <=
 * rec_end[r]: a CSR form, not an nrows x ncols table. oxh_csv_open_device reads the caller's d_bytes (any
 * alignment), which must stay alive and unchanged until oxh_csv_close; oxh_csv_open_host owns a device copy. All
 * entries block until complete. A handle is used by one thread at a time, on the device of its ctx; the ctx must
 * outlive it. stream (hipStream_t, NULL = the null stream) orders the device forms' work; the host forms,
 * oxh_csv_infer and oxh_csv_header use the ctx's stream.
 *   stats8 = {records, data rows, ncols, delimiters (the entries of `ends`), skipped empty records, short records,
 *   long records, 1 if the buffer ended inside quotes}.
 * oxh_csv_open_*: OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path), in this order: a separator above
 * 255; a quote above OXH_CSV_NO_QUOTE; a separator that is '\n' or '\r'; a quote that is '\n' or '\r'; a quote
 * equal to the separator; unknown flags; nbytes >= 2^32; NULL bytes with nbytes > 0; NULL out; NULL stats8; then
 * nbytes == 0 is OXH_OK with zeroed stats and a valid empty handle; then OXH_ERR_NODEVICE; then a NULL ctx. A
 * failed allocation is OXH_ERR_NOMEM with the outputs untouched.
 * oxh_csv_close: NULL is OXH_OK.
 * oxh_csv_header: the header's names one after the other in names (capacity bytes) with ncols + 1 name_offsets;
 * names_bytes always receives their size, and with names NULL or a capacity below it nothing else is written
 * (OXH_OK: the caller sizes and calls again). Without OXH_CSV_HAS_HEADER there are no names: 0 bytes, offsets 0.
 * OXH_ERR_INVALID: a NULL handle, name_offsets or names_bytes.
 * oxh_csv_infer: types[c] for the ncols columns. OXH_ERR_INVALID: a NULL handle; NULL types with ncols > 0.
 * max_rows == 0 or no rows: every column is OXH_CSV_STRING.
 * oxh_csv_columns_*: the nsel columns col_idx[k] (any order, repeats allowed) as types[k]. Outputs, per selection:
 * values (INT64 / FLOAT64: nrows 8-byte cells; BOOL: ceil(nrows / 8) bytes from bit 0; strings: the bytes),
 * offsets (strings: nrows + 1 int32 / int64 from 0; else not read), validity (ceil(nrows / 8) bytes, an Arrow
 * bitmap from bit 0, the bits past nrows zero, ALWAYS written). value_capacity[k] = the bytes values[k] holds.
 * value_bytes[k] = the bytes of values in use; stats4 (4 per selection) = {nulls from empty or missing fields,
 * nulls from unparsable text, deferred cells, value bytes}. With the three output tables NULL the call only
 * measures (value_bytes, stats4), as the take and the concat do, so the caller can size string buffers. In
 * _device the buffers the tables name are on the device, in _host on the host; the tables themselves,
 * value_capacity, value_bytes and stats4 are host arrays in both. OXH_ERR_INVALID, in this order: a NULL handle;
 * with selections NULL col_idx or types; a col_idx[k] >= ncols; an unknown type; NULL value_bytes or stats4; only
 * some of the three output tables NULL; outputs without value_capacity; with rows, per selection: a NULL
 * validity[k], a string column without offsets[k], with a capacity and no values[k] or with offsets[k] not aligned
 * to its 4- / 8-byte entries, another column without values[k], with a capacity below its values or (INT64, FLOAT64)
 * with values[k] not 8-byte aligned -- the alignments in both forms, as Arrow's buffers have them; then, after the
 * strings were measured and before anything is
 * written: an OXH_CSV_STRING column of more than 2^31 - 1 bytes, a string column above its value_capacity. nsel ==
 * 0 or no rows: OXH_OK, value_bytes and stats4 zeroed, nothing else written. A failed allocation is OXH_ERR_NOMEM
 * with the outputs untouched. */
#define OXH_CSV_NO_QUOTE 256
#define OXH_CSV_HAS_HEADER 1
#define OXH_CSV_INT64 1
#define OXH_CSV_FLOAT64 2
#define OXH_CSV_BOOL 3
#define OXH_CSV_STRING 4
#define OXH_CSV_STRING64 5
int oxh_csv_open_device(oxh_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, uint32_t separator, uint32_t quote, uint32_t flags,
                        void** out, uint64_t* stats8, void* stream);
int oxh_csv_open_host(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint32_t separator, uint32_t quote, uint32_t flags,
                      void** out, uint64_t* stats8);
int oxh_csv_close(void* csv);
int oxh_csv_header(void* csv, uint8_t* names, uint64_t capacity, uint64_t* name_offsets, uint64_t* names_bytes);
int oxh_csv_infer(void* csv, uint64_t max_rows, uint32_t* types);
int oxh_csv_columns_device(void* csv, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                           void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity, uint64_t* value_bytes,
                           uint64_t* stats4, void* stream);
int oxh_csv_columns_host(void* csv, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                         void* const* values, void* const* offsets, uint8_t* const* validity, uint64_t* value_bytes,
                         uint64_t* stats4);

/* ---------------------------------------------------------------- CSV text: typed Arrow columns to the file's bytes
 * Every path of the reference that produces a frame ends in `write_df` (core/df/tabular.rs:1492-1547): `oxen df
 * --output` / `--write` (command/df.rs:20,25,52), the diff's output (cmd/diff.rs:343, repositories/diffs.rs:1378), the
 * tabular merge, restore and checkout results (repositories/merge.rs:872, restore.rs:496, checkout.rs:182), the
 * workspace commit (repositories/workspaces/data_frames.rs:223) and oxen-py's df_utils.rs:19. oxh_write_csv_* do its
 * `csv` and `tsv` arms on the device: the columns of this header's own description (what oxh_csv_columns_* and every
 * tabular entry above produce) to the bytes of the file. (The oxh_csv_* names are the reader's seven entries over
 * its handle; the writer has no handle and is named by what it does.)
 *
 * The rules restate polars 0.49.1's CsvWriter as the reference configures it (include_header(true),
 * with_separator(delimiter), everything else default). They are NOT pinned by a run of polars.
 *   Records. The header record, when OXH_CSV_HAS_HEADER is set, holds the column names written by the string rule;
 *     one record per row follows; fields are joined by the one-byte separator; every record, the last one included,
 *     ends with '\n'. There is no BOM and no '\r'.
 *   Null cell (any type): no bytes.
 *   OXH_CSV_INT64    decimal digits, '-' in front of a negative, never '+'; INT64_MIN is -9223372036854775808.
 *   OXH_CSV_BOOL     true / false.
 *   OXH_CSV_FLOAT64  ryu's Buffer::format. A finite value: the shortest digits that read back as the value, nearest
 *     to it; with d those digits (L of them, no trailing zero), the value d x 10^k and kk = L + k:
 *       0 <= k and kk <= 16   digits, k zeros, ".0"         12.0 -> 12.0, 1e15 -> 1000000000000000.0
 *       0 < kk <= 16          the point after kk digits     12.5 -> 12.5
 *       -5 < kk <= 0          "0.", -kk zeros, digits       1e-5 -> 0.00001, 0.1 -> 0.1
 *       L == 1                d "e" (kk - 1)                1e16 -> 1e16, 1e-6 -> 1e-6
 *       otherwise             d0 "." rest "e" (kk - 1)      1.5e16 -> 1.5e16, 1.25e-7 -> 1.25e-7
 *     with no '+' and no zero padding in the exponent. The zeros are 0.0 and -0.0. Every NaN is NaN (no sign, no
 *     payload); the infinities are inf / -inf.
 *   OXH_CSV_STRING / OXH_CSV_STRING64 (the column is OXH_COL_BYTES32 / OXH_COL_BYTES64): quote style "necessary". A
 *     cell is quoted iff it is empty, or contains the separator, the quote byte, '\n' or '\r'; inside the quotes every
 *     quote byte is doubled; all other bytes are copied as they are (no UTF-8 check). An empty string is "" (two
 *     quote bytes): that keeps it apart from a null, and the reader's "Nulls" rule reads it back as an empty string.
 *   Floats on the device. The device writes a double itself where one IEEE division proves its shortest digits: a
 *     normal |v| < 1e15 whose digits are an integer m < 1e15 with |v| == double(m) / 10^j for a j in 0 .. 22, and the
 *     zeros, infinities and NaNs. Every other finite value is DEFERRED -- subnormals, |v| >= 1e15, doubles with 16 or
 *     17 shortest digits (the output of most arithmetic), digits further than 22 places behind the point: compacted
 *     in (row, column) order on the device, the bits brought down, formatted on the host (std::to_chars, then the
 *     same digits-to-text function) and copied into place inside the same blocking call. stats4[2] counts them; a
 *     column of such doubles pays a host conversion per cell.
 *   One column and a null. A one-column frame writes a null row as an empty record, which oxh_csv_open_* skips (its
 *     "Records" rule): reading the file back loses exactly those rows. Frames of two and more columns round-trip.
 *   Stated and not built: narrower integers and floats, dates, float_precision, other quote styles, a null_value.
 *
 * Inputs: nrows rows of ncols columns; types[c] (OXH_CSV_*) says how column c is written and kinds[c] (OXH_COL_*)
 * what its arrays are; values / offsets / validity / bit_offsets as oxh_row_hashes_* takes them; the column names
 * as bytes one after the other in names with ncols + 1 name_offsets (read only with OXH_CSV_HAS_HEADER; host memory
 * in both forms). Outputs: the file's bytes in out (capacity bytes; device memory in _device, host memory in _host);
 * out_bytes = the file's size; stats4 = {bytes, quoted cells (the header's included), deferred float cells, null
 * cells}. With out NULL the call only measures (out_bytes, stats4), as the take, the concat and oxh_csv_columns_* do.
 * With a capacity below the need nothing is written to out, out_bytes and stats4 are set and the call returns
 * OXH_ERR_INVALID. nrows == 0 writes the header alone. Both forms block until complete; stream (hipStream_t, NULL =
 * the null stream) orders the device form's work, the host form stages its columns through one device block and
 * uses the ctx's stream. A pair of offsets that is negative or decreases is never read through.
 * OXH_ERR_INVALID, before OXH_ERR_NODEVICE (there is no CPU path), in this order: NULL types, kinds, values, offsets,
 * validity or bit_offsets; ncols == 0; a separator above 255; a quote of OXH_CSV_NO_QUOTE (the writer always has a
 * quote byte) or above 255; a separator that is '\n' or '\r'; a quote that is '\n' or '\r'; a quote equal to the
 * separator; a separator, then a quote, that can occur in the text of a number or boolean (0-9, '+', '-', '.', the
 * ASCII letters); unknown flags; an unknown type; a column whose kind does not fit its type (INT64 / FLOAT64 need
 * OXH_COL_FIXED8, BOOL needs OXH_COL_BOOL, STRING needs OXH_COL_BYTES32, STRING64 needs OXH_COL_BYTES64); with
 * OXH_CSV_HAS_HEADER: NULL name_offsets, name_offsets that decrease, NULL names with name bytes; NULL out_bytes or
 * stats4; more than 2^40 rows; with rows, per column: a byte column without offsets, another column without values,
 * and in the host form offsets that are negative or decrease, bytes without values; then OXH_ERR_NODEVICE; then a
 * NULL ctx; then, after the lengths were measured and before anything is written: a pair of offsets that is negative
 * or decreases, a byte column with bytes and no values, a single row whose text is 2^32 bytes or more; then a
 * capacity below the need. A failed allocation is OXH_ERR_NOMEM with the outputs untouched. */
int oxh_write_csv_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                         const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                         const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint32_t separator,
                         uint32_t quote, uint32_t flags, uint8_t* d_out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4,
                         void* stream);
int oxh_write_csv_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                       const void* const* values, const void* const* offsets, const uint8_t* const* validity,
                       const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint32_t separator,
                       uint32_t quote, uint32_t flags, uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4);

/* ---------------------------------------------------------------- JSON text: typed Arrow columns to the file's bytes
 * The reference turns a frame into JSON at two places: `write_df`'s `jsonl`, `ndjson` and `json` arms
 * (core/df/tabular.rs:1469-1490, 1536-1538; JsonWriter with JsonFormat::JsonLines / JsonFormat::Json), and every
 * data-frame view the server returns (JsonDataFrameView::json_from_df, view/json_data_frame_view.rs:268-285, and
 * view/json_data_frame.rs:129: JsonWriter with JsonFormat::Json over the page). oxh_write_json_* do both on the
 * device, over the same columns as oxh_write_csv_*.
 *
 * The rules restate polars 0.49.1's JsonWriter (polars-json's serializers). They are NOT pinned by a run of polars.
 *   File shape. OXH_JSON_LINES (flags 0): one object per row, each followed by '\n', the last one too; zero rows
 *     give zero bytes. OXH_JSON_ARRAY (flag 1): '[', the rows' objects joined by ',', ']', with no newline anywhere;
 *     zero rows give []. A row is {"name":value,"name":value}: the columns in order, no spaces. A name is written by
 *     the string rule; the names are not checked for duplicates.
 *   Null cell (any type): null.
 *   OXH_CSV_INT64    the CSV rule: decimal digits, '-' in front of a negative.
 *   OXH_CSV_BOOL     true / false.
 *   OXH_CSV_FLOAT64  a finite value is ryu's Buffer::format, exactly the CSV rule's five forms, with 0.0 and -0.0;
 *     every NaN and both infinities are null.
 *   OXH_CSV_STRING / OXH_CSV_STRING64: '"', the bytes, '"'; an empty string is "". '"' becomes \" and '\' becomes
 *     \\; 0x08, 0x0C, 0x0A, 0x0D, 0x09 become \b, \f, \n, \r, \t; every other byte below 0x20 becomes \u00XX with
 *     lowercase hex; everything else is copied as it is -- 0x7F, '/' and every byte at or above 0x80. There is no
 *     UTF-8 check.
 *   The type codes are the OXH_CSV_* above: they are this header's only column-type enum, not the CSV format's own.
 *   Floats on the device: as in "CSV text". The doubles that one IEEE division does not prove are DEFERRED to the
 *     host inside the same blocking call, through the same 32-byte slots and the same conversion; stats4[2] counts
 *     them.
 *   Stated and not built: lists and embeddings (polars writes a float32 by its own shortest digits), structs, dates,
 *     narrower numbers, pretty printing.
 *
 * Inputs: as oxh_write_csv_* without separator and quote; names and name_offsets are always read (host memory in
 * both forms); flags is OXH_JSON_LINES or OXH_JSON_ARRAY. Outputs: the file's bytes in out (capacity bytes; device
 * memory in _device, host memory in _host); out_bytes = the file's size; stats4 = {bytes, string cells in which at
 * least one byte was escaped (a name that needs escaping counts once when the frame has rows), deferred float cells,
 * cells written as null (null cells and non-finite floats together)}. With out NULL the call only measures. With a
 * capacity below the need nothing is written to out, out_bytes and stats4 are set and the call returns
 * OXH_ERR_INVALID. Both forms block until complete; stream orders the device form's work, the host form stages its
 * columns through one device block and uses the ctx's stream. A pair of offsets that is negative or decreases is
 * never read through.
 * OXH_ERR_INVALID, every message starting with "json write:", before OXH_ERR_NODEVICE (there is no CPU path), in this
 * order: NULL types, kinds, values, offsets, validity or bit_offsets; ncols == 0; unknown flags; an unknown type; a
 * column whose kind does not fit its type; NULL name_offsets, name_offsets that decrease, NULL names with name bytes;
 * NULL out_bytes or stats4; more than 2^40 rows; with rows, per column: a byte column without offsets, another
 * column without values, and in the host form offsets that are negative or decrease, bytes without values; then
 * OXH_ERR_NODEVICE; then a NULL ctx; then, after the lengths were measured and before anything is written: a pair of
 * offsets that is negative or decreases, a byte column with bytes and no values, a single row whose text is 2^32
 * bytes or more; then a capacity below the need. A failed allocation is OXH_ERR_NOMEM with the outputs untouched. */
#define OXH_JSON_LINES 0
#define OXH_JSON_ARRAY 1
int oxh_write_json_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                          const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                          const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint32_t flags,
                          uint8_t* d_out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4, void* stream);
int oxh_write_json_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                        const void* const* values, const void* const* offsets, const uint8_t* const* validity,
                        const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint32_t flags,
                        uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4);

/* ---------------------------------------------------------------- JSON Lines: record index and typed Arrow columns
 * The reference has a JSON Lines arm in every reader: read_df_jsonl (core/df/tabular.rs:73-82), scan_df_jsonl
 * (:150-160) and the "ndjson" | "jsonl" arm of _read_lazy_df_with_extension (:1077-1079). oxh_jsonl_* do it on the
 * device: JSON Lines bytes in HBM to a record index (a handle), then to the same typed columns oxh_csv_columns_*
 * produce, which every tabular entry above takes as they are and oxh_write_json_* writes back.
 *
 * The rules restate polars' LazyJsonLineReader under the reference's settings (infer_schema_length 10 000). They
 * are NOT pinned by a run of polars; where this library chooses differently from polars, the rule says so.
 *   Records. The buffer splits at EVERY '\n', whatever the string state (a raw newline inside a string is not
 *     JSON). The end of the buffer ends the last record. JSON whitespace inside a record is 0x20, 0x09 and 0x0D, so
 *     a '\r' before the '\n' is just whitespace. A line of zero bytes or of whitespace only is skipped and counted.
 *     Every other line is a record and a row, well formed or not. A UTF-8 BOM is not skipped: it makes the first
 *     record malformed (out of scope).
 *   Lexing, from the start of each line (no state crosses a '\n'). A byte is ESCAPED iff the maximal run of '\'
 *     directly before it, inside the same line, has odd length. A '"' that is not escaped toggles "inside a
 *     string"; the line starts outside. Outside strings '{' and '[' add 1 to the depth, '}' and ']' subtract 1; the
 *     line starts at depth 0. A stray quote or bracket damages its own line only.
 *   Well-formed record. The first non-whitespace byte is '{' and the last is '}'; the depth is at least 1
 *     everywhere between them and returns to 0 exactly at that last byte; the line does not end inside a string;
 *     the structural bytes at depth 1 outside strings are "{ }" with only whitespace between, or "{ : , : , ... : }"
 *     in strict alternation that starts and ends with ':'; every key slot (from '{' or ',' to ':') is exactly one
 *     string token with whitespace around it; every value slot (from ':' to ',' or '}') is non-empty after trimming
 *     whitespace. The interior of a nested value is checked for depth and string state only: bracket kinds are NOT
 *     matched ("[}" passes). Every cell of a malformed record is null in every column; malformed records are counted.
 *   Value kinds, per cell, on the trimmed slot. First byte '"': a string token -- its last byte is an unescaped '"'
 *     and there is no other unescaped '"' inside; every '\' escape is one of \" \\ \/ \b \f \n \r \t \uXXXX (four
 *     hex digits, either case); no raw byte below 0x20; a high surrogate \uD800-\uDBFF is directly followed by a low
 *     one \uDC00-\uDFFF, and a lone surrogate of either kind is invalid; bytes at or above 0x80 are copied as they
 *     are, with no UTF-8 check, as the CSV reader does. First byte '{' or '[': a nested value, which ends with '}' or
 *     ']' respectively. true, false, null: exact, lower case. First byte '-' or a digit: the whole slot matches
 *     -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? . Anything else, or a token that breaks its own rule, is
 *     UNPARSABLE.
 *   Names (the schema). The keys in order of first appearance over the well-formed records among the first
 *     infer_rows rows. Keys are compared and reported UNESCAPED: "a\u0062" and "ab" are one column. A record is
 *     CANONICAL iff its keys are exactly the first k names, in order, for some k <= ncols. In a record with a
 *     repeated key the FIRST occurrence wins (this library's choice; simd-json's answer depends on the object's
 *     size). A field whose key is not a name is ignored and counted; it can only come after the window. At most
 *     65 535 names.
 *   Types (the OXH_CSV_* codes above, this header's only column-type enum). A missing key, null, or any cell of a
 *     malformed record is null in every type (stats4[0]).
 *     OXH_CSV_INT64    a number token without fraction or exponent, in the int64 range (-0 is 0). Every other token
 *                      is null and counted as unparsable (stats4[1]) -- 1.0 and 1e3 too: this library's choice.
 *     OXH_CSV_FLOAT64  any number token: the CORRECTLY ROUNDED double, bit for bit what C's strtod gives. -0 is
 *                      -0.0; a value out of range rounds to +-inf as strtod does; there are no inf / nan spellings.
 *                      The device converts where one IEEE operation is exact and defers the rest to the host inside
 *                      the same call, exactly as "CSV" above says; stats4[2] counts the deferred cells.
 *     OXH_CSV_BOOL     true / false.
 *     OXH_CSV_STRING / OXH_CSV_STRING64  a string token gives its unescaped bytes (each \uXXXX 1-3 bytes of UTF-8, a
 *                      surrogate pair 4; \u0000 is the byte 0x00). A number, true or false gives its text as written
 *                      (polars would re-print the number). A nested value gives its trimmed raw text, so a list of
 *                      floats or a metadata object survives as JSON text (polars makes a List / Struct). Unparsable
 *                      is null. The unescaped text is never longer than the raw text.
 *   Inference (oxh_jsonl_infer, over the same window). As the CSV rule: the AND of class bits, a null or missing
 *     cell having all three. Int64 if every cell is an integer in range, else Float64 if every cell is a number, else
 *     Boolean if every cell is a bool, else String; a column with no cell but nulls is String.
 *   Stated and not built: the `.json` array form (read_df_json: its records end by depth, not by line); lists and
 *     structs as typed columns, dates, narrower numbers; buffers of 2^32 bytes and more; files larger than one
 *     device buffer.
 *
 * The handle (a void*, as the CSV reader's) holds the index: `ends`, the u32 positions in ascending order of every
 * '\n' and of the bytes outside strings that open depth 1, close it, or are a ':' or ',' at depth 1 (4 B each);
 * `rec_end`, for every line the place of its end in `ends`; `row_rec`, the lines that are records; a bit per row for
 * "well formed" and for "canonical"; and the names. A well-formed record of k fields owns 2 k + 1 entries of `ends`
 * (2 for "{}"). A canonical row reads field c directly, any other row searches its keys from the front. Lifetime,
 * threading and streams are the CSV handle's: oxh_jsonl_open_device reads the caller's d_bytes (any alignment),
 * which must stay alive and unchanged until oxh_jsonl_close; oxh_jsonl_open_host owns a device copy; all entries
 * block until complete; a handle is used by one thread at a time; stream orders the device forms' work, the host
 * forms, oxh_jsonl_infer and oxh_jsonl_names use the ctx's stream. A line of whitespace only, and the whitespace
 * around a record, is walked by one lane. A string cell of 512 bytes and more without an escape is read and copied
 * by a whole wave; one with an escape is unescaped by one lane (exact, slower than the CSV reader's long cells).
 *   stats8 = {records, rows (= records), ncols, malformed records, skipped blank lines, well-formed rows that are
 *   not canonical, ignored fields, nested values at depth 1 (of well-formed records)}.
 * oxh_jsonl_open_*: infer_rows is the window (UINT64_MAX: every row; the reference passes 10 000). OXH_ERR_INVALID,
 * every message starting with "jsonl open:", before OXH_ERR_NODEVICE (there is no CPU path), in this order:
 * infer_rows == 0; unknown flags (none are defined); nbytes >= 2^32; NULL bytes with nbytes > 0; NULL out; NULL
 * stats8; then nbytes == 0 is OXH_OK with zeroed stats and a valid empty handle; then OXH_ERR_NODEVICE; then a NULL
 * ctx; after the index, more than 65 535 names is OXH_ERR_INVALID with nothing written. A failed allocation is
 * OXH_ERR_NOMEM with the outputs untouched.
 * oxh_jsonl_close: NULL is OXH_OK.
 * oxh_jsonl_names: the unescaped names, by the size-then-fill contract of oxh_csv_header.
 * oxh_jsonl_infer: types[c] for the ncols columns. OXH_ERR_INVALID: a NULL handle; NULL types with ncols > 0. No
 * rows: every column is OXH_CSV_STRING.
 * oxh_jsonl_columns_*: the parameters, outputs, measure-only mode, checks (in the same order) and stats4 of
 * oxh_csv_columns_*, word for word; stats4 = {nulls from null, a missing key or a malformed record, nulls from
 * unparsable cells, deferred cells, value bytes}. Messages start with "jsonl columns:". */
int oxh_jsonl_open_device(oxh_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, uint64_t infer_rows, uint32_t flags, void** out,
                          uint64_t* stats8, void* stream);
int oxh_jsonl_open_host(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint64_t infer_rows, uint32_t flags, void** out,
                        uint64_t* stats8);
int oxh_jsonl_close(void* jsonl);
int oxh_jsonl_names(void* jsonl, uint8_t* names, uint64_t capacity, uint64_t* name_offsets, uint64_t* names_bytes);
int oxh_jsonl_infer(void* jsonl, uint32_t* types);
int oxh_jsonl_columns_device(void* jsonl, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                             void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity, uint64_t* value_bytes,
                             uint64_t* stats4, void* stream);
int oxh_jsonl_columns_host(void* jsonl, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                           void* const* values, void* const* offsets, uint8_t* const* validity, uint64_t* value_bytes,
                           uint64_t* stats4);

/* ---------------------------------------------------------------- K2: merkle parent nodes */
/* get_combined_hash (hasher.rs:67-80) x n on the device:
 * XXH3-128(content.to_le_bytes() || metadata.to_le_bytes()), inputs as (lo, hi) pairs. */
int oxh_combined_hash_device(const uint64_t* d_content, const uint64_t* d_metadata, uint64_t n,
                             uint64_t* d_out, void* stream);
/* Host-resident batch of caller-serialised parent streams (vnode ids, commit_writer.rs:686-720;
 * dir hashes, commit_writer.rs:995-1147; metadata JSON, hasher.rs:95-100): item i is
 * streams[offsets[i] .. offsets[i] + lens[i]). Blocks until `out` (2n u64) is filled. */
int oxh_hash_streams(oxh_ctx* ctx, const uint8_t* streams, const uint64_t* offsets,
                     const uint64_t* lens, uint64_t n, uint64_t* out);

/* ---------------------------------------------------------------- multi-GPU: the digest gather
 * files shard across the GPUs of a node as contiguous byte-balanced ranges, one process
 * per GPU and no data-path collective; the one exchange is the 16-B-per-file digest table, gathered over
 * xGMI with RCCL. This replaces the reference's in-process fan-out of 64-file batches
 * (core/v_latest/add.rs:422-425) when the shards are device-resident on several GPUs.
 * RCCL is loaded at run time (librccl.so.1; $OXH_RCCL_LIB overrides); without it the calls fail with
 * OXH_ERR_NODEVICE.
 * One rank calls oxh_comm_unique_id and hands the OXH_COMM_ID_BYTES bytes to every rank out of band
 * (as ncclGetUniqueId); each rank then calls oxh_comm_create with its rank and GPU (it blocks until all
 * nranks have). oxh_gather_digests: counts[q] (host, nranks entries, the same on every rank) = rank q's
 * item count; rank q's d_local holds its 2 * counts[q] u64 digests (lo, hi); d_full (2 * sum(counts) u64,
 * device) receives every rank's table in rank order -- on every rank when root < 0 (all-gather), else on
 * rank `root` only (d_full may be NULL on the others). Equal counts take one ncclAllGather / ncclGather,
 * ragged ones a group of point-to-point transfers. Enqueued on `stream` (hipStream_t, NULL = the null
 * stream); returns without waiting. A communicator is used by one thread at a time.
 * oxh_comm_check: OXH_OK when RCCL loads and `device` is a visible HIP device, else the error
 * oxh_comm_create would return for that reason (OXH_ERR_NODEVICE / OXH_ERR_INVALID) without joining
 * anything -- every rank calls it and the job agrees on the result before any rank enters
 * oxh_comm_create, which would otherwise wait in RCCL's bootstrap for a rank that has already failed. */
#define OXH_COMM_ID_BYTES 128
typedef struct oxh_comm oxh_comm;
int oxh_comm_check(int device);
int oxh_comm_unique_id(uint8_t* id);
int oxh_comm_create(const uint8_t* id, int rank, int nranks, int device, oxh_comm** out);
int oxh_comm_info(oxh_comm* comm, int* rank, int* nranks, int* device);
int oxh_gather_digests(oxh_comm* comm, const uint64_t* d_local, const uint64_t* counts, uint64_t* d_full, int root,
                       void* stream);
int oxh_comm_destroy(oxh_comm* comm);

/* ---------------------------------------------------------------- formatting (host only) */
/* MerkleHash Display (merkle_hash.rs:73-77): format!("{:x}") -- lowercase, NOT zero-padded.
 * `out` must hold 33 bytes; returns the string length (1..32). */
int oxh_format_hex(uint64_t lo, uint64_t hi, char* out);
/* u128::to_string() -- the decimal chunk names of the dedup experiment (fixedsize.rs:78).
 * `out` must hold 40 bytes; returns the string length. */
int oxh_format_dec(uint64_t lo, uint64_t hi, char* out);

/* ---------------------------------------------------------------- bench / test utilities */
/* Fill d_buf[0..nbytes) with the counter-based splitmix64 byte stream of `seed` (byte j is byte
 * j%8, little-endian, of splitmix64(seed + (j/8 + 1) * 0x9E3779B97F4A7C15)) so that a host can
 * regenerate any item of a device-resident synthetic workload without copying it back. */
int oxh_fill_splitmix(void* d_buf, uint64_t nbytes, uint64_t seed, void* stream);
/* Diagnostic: select the long-path kernel variant (0 = default). Returns the previous value. */
int oxh_set_kernel_variant(int variant);
/* Diagnostic: byte in 0..255 = fill every working allocation of a call with it before the call uses it;
 * -1 (default) = off. Returns the previous value. */
int oxh_set_scratch_poison(int byte);
/* Diagnostic: bytes filled so far under a poison (device and pinned together). */
uint64_t oxh_scratch_poisoned_bytes(void);
/* Diagnostic counters of a context, out[0..n): [0] device allocations of the large-file piece buffers
 * (files above a staging slot; each one synchronises the device), [1] their current bytes, [2] file
 * requests served on the caller's thread (small requests on an idle context), [3] file-engine runs,
 * [4] staged slots submitted (host batches of files, buffers or streams), [5] the most items of 1 MiB
 * and more that one of those slots held (K1L takes the 32 largest of a slot); further entries 0. */
int oxh_ctx_counters(oxh_ctx* ctx, uint64_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* OXEN_HASH_H */
