// oxen_amd/csrc/capi_dispatch.hip -- K1 launch shapes and the device-resident entry points of the C ABI
// (include/oxen_hash.h): HBM in, HBM out, asynchronous on the caller's stream; errors and the ABI's
// library-level calls. The other runtime pieces are listed in capi_internal.hpp.
#include "capi_internal.hpp"

using namespace oxh::capi;

namespace oxh::capi {

thread_local std::string g_err;
std::atomic<int> g_variant{0};
}  // namespace oxh::capi

namespace oxh {
std::atomic<int> g_scratch_poison{-1};
std::atomic<uint64_t> g_scratch_poisoned{0};
}  // namespace oxh

namespace oxh::capi {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ---------------------------------------------------------------- kernel launch helpers
using WaveKernel = void (*)(const uint8_t*, const uint64_t*, const uint64_t*, uint64_t, uint64_t, uint64_t, uint64_t*);

// The shapes the dispatch below picks; any other forced variant runs the 4-round ring (Cfg<0>) with
// the launch geometry of one item per wave (known_variant). What each number is: Cfg, xxh3_kernels.hip.
template <bool DESC>
WaveKernel wave_kernel_for(int variant) {
    switch (variant) {
        case kVariantShort: return oxh::xxh3_wave_kernel<DESC, kVariantShort>;
        case kVariantLong: return oxh::xxh3_wave_kernel<DESC, kVariantLong>;
        case kVariantPacked: return oxh::xxh3_wave_kernel<DESC, kVariantPacked>;
        case kVariantRows: return oxh::xxh3_wave_kernel<DESC, kVariantRows>;
        default: return oxh::xxh3_wave_kernel<DESC, 0>;
    }
}

// K1 register/pipeline shape by item size (measured): items of a few KiB want many
// resident waves (2-round ring, keys in LDS, every load issued up front); larger items a 2-round ring
// with the keys in registers (variant 8). The 4-round ring (variant 0) matches it on equal 64 KiB
// items but loses 13 % on ragged, packed items (FastCDC chunks: tools/k1_align_probe.py) and 4 % of
// the C2 step rate. An explicit oxh_set_kernel_variant() overrides the choice.
//
// Items packed back to back (FastCDC chunks) start at arbitrary byte offsets: a row-wise
// instruction (256 B per row) then touches 3 lines where an aligned one touches 2, 12 lines per KiB
// instead of 8, which costs 6-8 % at 8-64 KiB items; the block-wise layout (variant bit 5) reads a
// whole KiB per instruction, 9 lines. tools/k1_small_probe.py (profiles/r02_k1_small_probe.json):
// packed [4, 16) KiB items 6.17-6.23 TB/s block-wise vs 5.90-5.93 row-wise, packed [4, 128) KiB
// 6.72 vs 6.25; on aligned items the row-wise variants stay ahead (6.75 vs 6.66 at 8 KiB).
// (kShortItemBytes, the variant numbers and ItemShape: capi_internal.hpp)
int pick_variant(ItemShape shape) {
    const int v = g_variant.load();
    if (v != 0) return v;
    return shape == ItemShape::Packed ? kVariantPacked : shape == ItemShape::Short ? kVariantShort : kVariantLong;
}
int pick_variant(bool short_items) { return pick_variant(short_items ? ItemShape::Short : ItemShape::Long); }
// a variant wave_kernel_for has a case for, else 0 (its default kernel), so the launch geometry always
// matches the kernel that runs
int known_variant(int v) {
    return (v == kVariantShort || v == kVariantLong || v == kVariantPacked || v == kVariantRows) ? v : 0;
}
// K1R hashes four items per wave, one per 16-lane row
uint64_t items_per_wave(int variant) { return variant == kVariantRows ? 4 : 1; }

// K1 over a descriptor table: one 64-lane wave per item, 4 waves per 256-thread workgroup.
int launch_wave(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens, uint64_t n, uint64_t* out,
                hipStream_t st, ItemShape shape, int waves, int variant) {
    if (n == 0) return OXH_OK;
    // waves (items) per workgroup: 4, or the caller's choice; OXH_K1_WG_WAVES (1, 2 or 4) overrides
    // both for A/B. A workgroup's slot is freed only when its longest item is done.
    const int e = oxh::env::k1_wg_waves();
    const int w = e ? e : (waves == 1 || waves == 2) ? waves : 4;
    const int v = known_variant((variant && g_variant.load() == 0) ? variant : pick_variant(shape));
    const uint64_t per_wg = (uint64_t)w * items_per_wave(v);
    const uint64_t blocks = (n + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(wave_kernel_for<true>(v), dim3((unsigned)blocks), dim3(64 * w), 0, st, arena, offs,
                       lens, n, (uint64_t)0, (uint64_t)0, out);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

// K1T: K1 plus text counts in the same pass.
int launch_text(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens, uint64_t n, uint64_t* out,
                uint64_t* counts, hipStream_t st) {
    if (n == 0) return OXH_OK;
    const uint64_t blocks = (n + 3) / 4;
    // K1T keeps the 2-round ring with the keys in LDS at every item size: the counting needs the
    // registers (tools/k1t_probe.py: 6.41 TB/s on C2 and 5.55 on ragged items, against 5.42 / 4.40
    // with variant 8 and 4.32 / 2.56 with the 4-round ring); only that shape ships
    hipLaunchKernelGGL(oxh::xxh3_text_wave_kernel<kVariantShort>, dim3((unsigned)blocks), dim3(256), 0, st, arena, offs, lens,
                       n, out, counts);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

// Fixed-size chunks of one buffer (no descriptor table): chunk i = [i*chunk, min((i+1)*chunk, total)).
int launch_chunks(const uint8_t* buf, uint64_t n, uint64_t chunk, uint64_t total, uint64_t* out, hipStream_t st) {
    if (n == 0) return OXH_OK;
    const int v = known_variant(pick_variant(chunk <= kShortItemBytes));
    const uint64_t per_wg = 4 * items_per_wave(v);
    const uint64_t blocks = (n + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(wave_kernel_for<false>(v), dim3((unsigned)blocks), dim3(256), 0, st, buf,
                       (const uint64_t*)nullptr, (const uint64_t*)nullptr, n, chunk, total, out);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

int launch_lane(const uint8_t* arena, const uint64_t* offs, const uint64_t* lens, uint64_t n, uint64_t* out,
                hipStream_t st) {
    if (n == 0) return OXH_OK;
    hipLaunchKernelGGL(oxh::xxh3_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, arena, offs, lens, n, out);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

}  // namespace oxh::capi

namespace oxh {
// FastCDC's K1 pass (fastcdc.hip) over the packed chunk table. Below a 16 KiB mean chunk K1R (four
// chunks per wave, one per 16-lane row: tools/k1_small_probe.py, profiles/r04g_k1_small_probe.json),
// otherwise the block-wise K1 (one chunk per wave; K1R's four streams per wave lose 10 % on 16-128 KiB
// items); 2 waves per workgroup below 16 KiB, else 4. oxh_set_kernel_variant overrides the shape
// (launch_wave).
int k1_packed(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens, uint64_t n, uint64_t* d_out,
              uint64_t mean_len, hipStream_t st) {
    const bool small = mean_len < kShortItemBytes;
    return launch_wave((const uint8_t*)d_arena, d_offsets, d_lens, n, d_out, st, ItemShape::Packed, small ? 2 : 4,
                       small ? kVariantRows : kVariantPacked);
}
}  // namespace oxh

extern "C" {

int oxh_abi_version(void) { return OXH_ABI_VERSION; }

const char* oxh_last_error(void) { return g_err.c_str(); }

int oxh_device_count(int* count) {
    if (!count) return fail(OXH_ERR_INVALID, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return OXH_OK;
}

int oxh_set_kernel_variant(int variant) { return g_variant.exchange(variant); }

int oxh_set_scratch_poison(int byte) { return oxh::g_scratch_poison.exchange(byte < 0 || byte > 255 ? -1 : byte); }

uint64_t oxh_scratch_poisoned_bytes(void) { return oxh::g_scratch_poisoned.load(); }

int oxh_xxh3_128_batch_device(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens, uint64_t n,
                              uint64_t* d_out, int mode, void* stream) {
    if (n == 0) return OXH_OK;
    if (!d_arena || !d_offsets || !d_lens || !d_out) return fail(OXH_ERR_INVALID, "NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* a = (const uint8_t*)d_arena;
    if (mode == OXH_MODE_LANE) return launch_lane(a, d_offsets, d_lens, n, d_out, st);
    if (mode == OXH_MODE_AUTO || mode == OXH_MODE_WAVE) return launch_wave(a, d_offsets, d_lens, n, d_out, st);
    if (mode == OXH_MODE_WAVE_SHORT) return launch_wave(a, d_offsets, d_lens, n, d_out, st, ItemShape::Short);
    if (mode == OXH_MODE_WAVE_PACKED) return launch_wave(a, d_offsets, d_lens, n, d_out, st, ItemShape::Packed);
    return fail(OXH_ERR_INVALID, "unknown mode");
}

int oxh_chunk_digests_device(const void* d_buf, uint64_t len, uint64_t chunk, uint64_t* d_out, void* stream) {
    if (len == 0) return OXH_OK;
    if (!d_buf || !d_out || chunk == 0) return fail(OXH_ERR_INVALID, "bad chunk arguments");
    return launch_chunks((const uint8_t*)d_buf, (len + chunk - 1) / chunk, chunk, len, d_out, (hipStream_t)stream);
}

int oxh_xxh3_128_large_device(oxh_ctx* c, const void* d_buf, uint64_t len, uint64_t* d_out, void* stream) {
    if (!c || !d_out || (!d_buf && len)) return fail(OXH_ERR_INVALID, "bad large-buffer arguments");
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the null stream, as for every device entry point
    return large_device(c, (const uint8_t*)d_buf, len, d_out, st);
}

int oxh_xxh3_128_large_batch_device(const void* const* d_bufs, const uint64_t* lens, uint64_t n, uint64_t* d_out,
                                    void* stream) {
    if (n == 0) return OXH_OK;
    if (!d_bufs || !lens || !d_out) return fail(OXH_ERR_INVALID, "bad large-batch arguments");
    for (uint64_t i = 0; i < n; ++i)
        if (!d_bufs[i] && lens[i]) return fail(OXH_ERR_INVALID, "NULL buffer with nonzero length");
    return large_batch_device((const uint8_t* const*)d_bufs, lens, n, d_out, (hipStream_t)stream);
}

int oxh_combined_hash_device(const uint64_t* d_content, const uint64_t* d_metadata, uint64_t n, uint64_t* d_out,
                             void* stream) {
    if (n == 0) return OXH_OK;
    if (!d_content || !d_metadata || !d_out) return fail(OXH_ERR_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(oxh::xxh3_combined_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_content, d_metadata, n, d_out);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

int oxh_xxh3_128_text_batch_device(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens, uint64_t n,
                                   uint64_t* d_out, uint64_t* d_counts, void* stream) {
    if (n == 0) return OXH_OK;
    if (!d_arena || !d_offsets || !d_lens || !d_out || !d_counts) return fail(OXH_ERR_INVALID, "NULL device pointer");
    return launch_text((const uint8_t*)d_arena, d_offsets, d_lens, n, d_out, d_counts, (hipStream_t)stream);
}

int oxh_utf8_prefix_device(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens, uint64_t n,
                           int32_t* d_flags, void* stream) {
    if (n == 0) return OXH_OK;
    if (!d_arena || !d_offsets || !d_lens || !d_flags) return fail(OXH_ERR_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(oxh::utf8_prefix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)d_arena, d_offsets, d_lens, n, d_flags);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

int oxh_fill_splitmix(void* d_buf, uint64_t nbytes, uint64_t seed, void* stream) {
    if (!d_buf && nbytes) return fail(OXH_ERR_INVALID, "NULL buffer");
    if ((reinterpret_cast<uintptr_t>(d_buf) & 7) != 0) return fail(OXH_ERR_INVALID, "buffer must be 8-byte aligned");
    const uint64_t nwords = nbytes / 8;
    if (nwords) {
        const uint64_t blocks = std::min<uint64_t>((nwords + 255) / 256, 256ull * 64);
        hipLaunchKernelGGL(oxh::fill_splitmix_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           (uint64_t*)d_buf, nwords, seed);
        HIP_TRY(hipGetLastError());
    }
    if (nbytes % 8) {
        hipLaunchKernelGGL(oxh::fill_splitmix_tail_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream,
                           (uint8_t*)d_buf + nwords * 8, nwords, nbytes % 8, seed);
        HIP_TRY(hipGetLastError());
    }
    return OXH_OK;
}

// ---------------------------------------------------------------- Snappy (the kernel: snappy_inflate.hip)
static int snappy_args(uint64_t nblocks, const void* src, const void* src_offsets, const void* dst_offsets, const void* status,
                       const uint64_t* bad_blocks) {
    if (!bad_blocks) return fail(OXH_ERR_INVALID, "snappy inflate: bad_blocks is NULL");
    if (nblocks == 0) return OXH_OK;
    if (nblocks > 0xFFFFFFFFull) return fail(OXH_ERR_INVALID, "snappy inflate: more than 2^32 blocks");
    if (!src) return fail(OXH_ERR_INVALID, "snappy inflate: src is NULL");
    if (!src_offsets) return fail(OXH_ERR_INVALID, "snappy inflate: src_offsets is NULL");
    if (!dst_offsets) return fail(OXH_ERR_INVALID, "snappy inflate: dst_offsets is NULL");
    if (!status) return fail(OXH_ERR_INVALID, "snappy inflate: status is NULL");
    return OXH_OK;
}

static int snappy_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "snappy inflate: ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

int oxh_snappy_inflate_device(oxh_ctx* ctx, uint64_t nblocks, const uint8_t* d_src, const uint64_t* d_src_offsets, uint8_t* d_dst,
                              const uint64_t* d_dst_offsets, uint32_t* d_status, uint64_t* bad_blocks, void* stream) {
    int rc = snappy_args(nblocks, d_src, d_src_offsets, d_dst_offsets, d_status, bad_blocks);
    if (rc) return rc;
    if (nblocks == 0) return *bad_blocks = 0, OXH_OK;
    if ((rc = snappy_enter(ctx))) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* d_bad = nullptr;
    if (hipMalloc(&d_bad, 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "snappy inflate: 8 B for the count on the device");
    }
    unsigned long long bad = 0;
    rc = [&]() -> int {
        int r = oxh::snappy_inflate_enqueue(d_src, d_src_offsets, d_src_offsets + 1, d_dst, d_dst_offsets, d_dst_offsets + 1, d_status, nblocks,
                                            d_bad, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_bad);
    if (rc == OXH_OK) *bad_blocks = bad;
    return rc;
}

int oxh_snappy_inflate_host(oxh_ctx* ctx, uint64_t nblocks, const uint8_t* src, const uint64_t* src_offsets, uint8_t* dst,
                            const uint64_t* dst_offsets, uint32_t* status, uint64_t* bad_blocks) {
    int rc = snappy_args(nblocks, src, src_offsets, dst_offsets, status, bad_blocks);
    if (rc) return rc;
    if (nblocks == 0) return *bad_blocks = 0, OXH_OK;
    for (uint64_t b = 0; b < nblocks; ++b) {
        if (src_offsets[b + 1] < src_offsets[b]) return fail(OXH_ERR_INVALID, "snappy inflate: src_offsets decrease at block " + std::to_string(b));
        if (dst_offsets[b + 1] < dst_offsets[b]) return fail(OXH_ERR_INVALID, "snappy inflate: dst_offsets decrease at block " + std::to_string(b));
    }
    const uint64_t src_lo = src_offsets[0], src_bytes = src_offsets[nblocks] - src_lo, dst_lo = dst_offsets[0], dst_bytes = dst_offsets[nblocks] - dst_lo;
    if (dst_bytes && !dst) return fail(OXH_ERR_INVALID, "snappy inflate: dst is NULL");
    if ((rc = snappy_enter(ctx))) return rc;
    hipStream_t st = ctx->stream;
    // one device block: the input, the output, both offset tables from 0, the statuses, the count
    const uint64_t up16 = 15, at_dst = (src_bytes + up16) & ~up16, at_so = at_dst + ((dst_bytes + up16) & ~up16), at_do = at_so + (nblocks + 1) * 8,
                   at_status = at_do + (nblocks + 1) * 8, at_bad = (at_status + nblocks * 4 + 7) & ~7ull, total = at_bad + 8;
    std::vector<uint64_t> tables;
    try {
        tables.resize(2 * (nblocks + 1));
    } catch (const std::bad_alloc&) {
        return fail(OXH_ERR_NOMEM, "snappy inflate: the offset tables on the host");
    }
    for (uint64_t b = 0; b <= nblocks; ++b) tables[b] = src_offsets[b] - src_lo, tables[nblocks + 1 + b] = dst_offsets[b] - dst_lo;
    uint8_t* d = nullptr;
    if (hipMalloc(&d, total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "snappy inflate: " + std::to_string(total) + " B for the blocks on the device");
    }
    oxh::poison_device(d, total, st);
    std::vector<uint32_t> got(nblocks);
    unsigned long long bad = 0;
    rc = [&]() -> int {
        if (src_bytes) HIP_TRY(hipMemcpyAsync(d, src + src_lo, src_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + at_so, tables.data(), tables.size() * 8, hipMemcpyHostToDevice, st));
        const uint64_t *d_so = (const uint64_t*)(d + at_so), *d_do = (const uint64_t*)(d + at_do);
        int r = oxh::snappy_inflate_enqueue(d, d_so, d_so + 1, d + at_dst, d_do, d_do + 1, (uint32_t*)(d + at_status), nblocks,
                                            (unsigned long long*)(d + at_bad), st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(got.data(), d + at_status, nblocks * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&bad, d + at_bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // the caller's arrays stay untouched unless everything succeeded
        if (dst_bytes) HIP_TRY(hipMemcpy(dst + dst_lo, d + at_dst, dst_bytes, hipMemcpyDeviceToHost));
        memcpy(status, got.data(), nblocks * 4);
        *bad_blocks = bad;
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    return rc;
}

// ---------------------------------------------------------------- Zstandard (the kernel: zstd_inflate.hip)
static int zstd_args(uint64_t nblocks, const void* src, const void* src_offsets, const void* dst_offsets, const void* status,
                     const uint64_t* bad_blocks) {
    if (!bad_blocks) return fail(OXH_ERR_INVALID, "zstd inflate: bad_blocks is NULL");
    if (nblocks == 0) return OXH_OK;
    if (nblocks > 0xFFFFFFFFull) return fail(OXH_ERR_INVALID, "zstd inflate: more than 2^32 blocks");
    if (!src) return fail(OXH_ERR_INVALID, "zstd inflate: src is NULL");
    if (!src_offsets) return fail(OXH_ERR_INVALID, "zstd inflate: src_offsets is NULL");
    if (!dst_offsets) return fail(OXH_ERR_INVALID, "zstd inflate: dst_offsets is NULL");
    if (!status) return fail(OXH_ERR_INVALID, "zstd inflate: status is NULL");
    return OXH_OK;
}

static int zstd_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "zstd inflate: ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

int oxh_zstd_inflate_device(oxh_ctx* ctx, uint64_t nblocks, const uint8_t* d_src, const uint64_t* d_src_offsets, uint8_t* d_dst,
                            const uint64_t* d_dst_offsets, uint32_t* d_status, uint64_t* bad_blocks, void* stream) {
    int rc = zstd_args(nblocks, d_src, d_src_offsets, d_dst_offsets, d_status, bad_blocks);
    if (rc) return rc;
    if (nblocks == 0) return *bad_blocks = 0, OXH_OK;
    if ((rc = zstd_enter(ctx))) return rc;
    hipStream_t st = (hipStream_t)stream;
    oxh::ScratchLease lease(st);  // the waves' literal slots, then the count
    const uint64_t at_bad = oxh::zstd_slot_bytes(nblocks), total = at_bad + 8;
    void* base = nullptr;
    if (lease.get(total, &base) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "zstd inflate: " + std::to_string(total) + " B of literal slots on the device");
    }
    uint8_t* d = (uint8_t*)base;
    unsigned long long bad = 0;
    rc = [&]() -> int {
        int r = oxh::zstd_inflate_enqueue(d_src, d_src_offsets, d_src_offsets + 1, d_dst, d_dst_offsets, d_dst_offsets + 1, d_status, nblocks, d,
                                          (unsigned long long*)(d + at_bad), st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(&bad, d + at_bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    if (rc == OXH_OK) *bad_blocks = bad;
    return rc;
}

int oxh_zstd_inflate_host(oxh_ctx* ctx, uint64_t nblocks, const uint8_t* src, const uint64_t* src_offsets, uint8_t* dst,
                          const uint64_t* dst_offsets, uint32_t* status, uint64_t* bad_blocks) {
    int rc = zstd_args(nblocks, src, src_offsets, dst_offsets, status, bad_blocks);
    if (rc) return rc;
    if (nblocks == 0) return *bad_blocks = 0, OXH_OK;
    for (uint64_t b = 0; b < nblocks; ++b) {
        if (src_offsets[b + 1] < src_offsets[b]) return fail(OXH_ERR_INVALID, "zstd inflate: src_offsets decrease at block " + std::to_string(b));
        if (dst_offsets[b + 1] < dst_offsets[b]) return fail(OXH_ERR_INVALID, "zstd inflate: dst_offsets decrease at block " + std::to_string(b));
    }
    const uint64_t src_lo = src_offsets[0], src_bytes = src_offsets[nblocks] - src_lo, dst_lo = dst_offsets[0], dst_bytes = dst_offsets[nblocks] - dst_lo;
    if (dst_bytes && !dst) return fail(OXH_ERR_INVALID, "zstd inflate: dst is NULL");
    if ((rc = zstd_enter(ctx))) return rc;
    hipStream_t st = ctx->stream;
    // one device block: the input, the output, both offset tables from 0, the statuses, the count, the literal slots
    const uint64_t up16 = 15, at_dst = (src_bytes + up16) & ~up16, at_so = at_dst + ((dst_bytes + up16) & ~up16), at_do = at_so + (nblocks + 1) * 8,
                   at_status = at_do + (nblocks + 1) * 8, at_bad = (at_status + nblocks * 4 + 7) & ~7ull, at_slots = (at_bad + 8 + up16) & ~up16,
                   total = at_slots + oxh::zstd_slot_bytes(nblocks);
    std::vector<uint64_t> tables;
    try {
        tables.resize(2 * (nblocks + 1));
    } catch (const std::bad_alloc&) {
        return fail(OXH_ERR_NOMEM, "zstd inflate: the offset tables on the host");
    }
    for (uint64_t b = 0; b <= nblocks; ++b) tables[b] = src_offsets[b] - src_lo, tables[nblocks + 1 + b] = dst_offsets[b] - dst_lo;
    uint8_t* d = nullptr;
    if (hipMalloc(&d, total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "zstd inflate: " + std::to_string(total) + " B for the blocks on the device");
    }
    oxh::poison_device(d, total, st);
    std::vector<uint32_t> got(nblocks);
    unsigned long long bad = 0;
    rc = [&]() -> int {
        if (src_bytes) HIP_TRY(hipMemcpyAsync(d, src + src_lo, src_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + at_so, tables.data(), tables.size() * 8, hipMemcpyHostToDevice, st));
        const uint64_t *d_so = (const uint64_t*)(d + at_so), *d_do = (const uint64_t*)(d + at_do);
        int r = oxh::zstd_inflate_enqueue(d, d_so, d_so + 1, d + at_dst, d_do, d_do + 1, (uint32_t*)(d + at_status), nblocks, d + at_slots,
                                          (unsigned long long*)(d + at_bad), st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(got.data(), d + at_status, nblocks * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&bad, d + at_bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // the caller's arrays stay untouched unless everything succeeded
        if (dst_bytes) HIP_TRY(hipMemcpy(dst + dst_lo, d + at_dst, dst_bytes, hipMemcpyDeviceToHost));
        memcpy(status, got.data(), nblocks * 4);
        *bad_blocks = bad;
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    return rc;
}

// ---------------------------------------------------------------- Snappy, compress (the kernels: snappy_compress.hip)
uint64_t oxh_snappy_bound(uint64_t n) { return oxh::snappy_bound(n); }

static int snappy_compress_args(uint64_t nblocks, const void* src, const void* src_offsets, const void* dst_offsets, const void* sizes,
                                const void* status) {
    if (nblocks > 0xFFFFFFFFull) return fail(OXH_ERR_INVALID, "snappy compress: more than 2^32 blocks");
    if (!src) return fail(OXH_ERR_INVALID, "snappy compress: src is NULL");
    if (!src_offsets) return fail(OXH_ERR_INVALID, "snappy compress: src_offsets is NULL");
    if (!dst_offsets) return fail(OXH_ERR_INVALID, "snappy compress: dst_offsets is NULL");
    if (!sizes) return fail(OXH_ERR_INVALID, "snappy compress: sizes is NULL");
    if (!status) return fail(OXH_ERR_INVALID, "snappy compress: status is NULL");
    return OXH_OK;
}

static int snappy_compress_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "snappy compress: ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

namespace {
// The fragments of a call, from the offset tables on the host: good[b] = the block is compressed (its offsets do
// not decrease and its destination holds snappy_bound() of it); frag0 and frag_block as SnappyWork wants them.
struct SnappyPlan {
    std::vector<uint8_t> good;
    std::vector<uint64_t> frag0;
    std::vector<uint32_t> frag_block;
};

int snappy_plan(uint64_t nblocks, const uint64_t* src_offsets, const uint64_t* dst_offsets, SnappyPlan& p) {
    try {
        p.good.assign(nblocks, 0), p.frag0.assign(nblocks + 1, 0);
        for (uint64_t b = 0; b < nblocks; ++b) {
            p.frag0[b] = p.frag_block.size();
            if (src_offsets[b + 1] < src_offsets[b] || dst_offsets[b + 1] < dst_offsets[b]) continue;
            const uint64_t n = src_offsets[b + 1] - src_offsets[b];
            if (n > 0xFFFFFFFFull)
                return fail(OXH_ERR_INVALID, "snappy compress: block " + std::to_string(b) + " has " + std::to_string(n) + " B: more than 2^32 - 1");
            if (dst_offsets[b + 1] - dst_offsets[b] < oxh::snappy_bound(n)) continue;
            p.good[b] = 1;
            p.frag_block.insert(p.frag_block.end(), oxh::snappy_fragments(n), (uint32_t)b);
        }
        p.frag0[nblocks] = p.frag_block.size();
    } catch (const std::bad_alloc&) {
        return fail(OXH_ERR_NOMEM, "snappy compress: the fragment tables on the host");
    }
    return OXH_OK;
}

using oxh::SnappyLayout;

// The tables go up and every fragment is compressed into its slot.
int snappy_run_fragments(const SnappyPlan& p, const SnappyLayout& lay, uint8_t* d, const uint8_t* d_src, const uint64_t* d_src_lo,
                         const uint64_t* d_src_hi, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(d + lay.at_frag0, p.frag0.data(), p.frag0.size() * 8, hipMemcpyHostToDevice, st));
    if (!p.frag_block.empty()) HIP_TRY(hipMemcpyAsync(d + lay.at_block, p.frag_block.data(), p.frag_block.size() * 4, hipMemcpyHostToDevice, st));
    return oxh::snappy_fragments_enqueue(d_src, d_src_lo, d_src_hi, lay.work(d, p.frag_block.size()), st);
}

int snappy_ctrl_error(unsigned long long ctrl) {
    return ctrl ? fail(OXH_ERR_HIP, "snappy compress: a fragment's stream is not what the tables say (did the input change during the call?)") : OXH_OK;
}
}  // namespace

int oxh_snappy_compress_device(oxh_ctx* ctx, uint64_t nblocks, const uint8_t* d_src, const uint64_t* d_src_offsets, uint8_t* d_dst,
                               const uint64_t* d_dst_offsets, uint64_t* d_sizes, uint32_t* d_status, void* stream) {
    if (nblocks == 0) return OXH_OK;
    int rc = snappy_compress_args(nblocks, d_src, d_src_offsets, d_dst_offsets, d_sizes, d_status);
    if (rc) return rc;
    if (!d_dst) return fail(OXH_ERR_INVALID, "snappy compress: dst is NULL");
    if ((rc = snappy_compress_enter(ctx))) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the offset tables come down: the fragments are cut on the host
    std::vector<uint64_t> tables;
    try {
        tables.resize(2 * (nblocks + 1));
    } catch (const std::bad_alloc&) {
        return fail(OXH_ERR_NOMEM, "snappy compress: the offset tables on the host");
    }
    HIP_TRY(hipMemcpyAsync(tables.data(), d_src_offsets, (nblocks + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(tables.data() + nblocks + 1, d_dst_offsets, (nblocks + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    SnappyPlan plan;
    if ((rc = snappy_plan(nblocks, tables.data(), tables.data() + nblocks + 1, plan))) return rc;
    const SnappyLayout lay(0, nblocks, plan.frag_block.size());
    oxh::ScratchLease lease(st);
    void* base = nullptr;
    if (lease.get(lay.total, &base) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "snappy compress: " + std::to_string(lay.total) + " B of fragment slots on the device");
    }
    uint8_t* d = (uint8_t*)base;
    unsigned long long ctrl = 0;
    if ((rc = snappy_run_fragments(plan, lay, d, d_src, d_src_offsets, d_src_offsets + 1, st))) return rc;
    if ((rc = oxh::snappy_pack_enqueue(d_src_offsets, d_src_offsets + 1, d_dst, d_dst_offsets, d_dst_offsets + 1, d_sizes, d_status, nblocks, true,
                                       lay.work(d, plan.frag_block.size()), st)))
        return rc;
    HIP_TRY(hipMemcpyAsync(&ctrl, d + lay.at_ctrl, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return snappy_ctrl_error(ctrl);
}

int oxh_snappy_compress_host(oxh_ctx* ctx, uint64_t nblocks, const uint8_t* src, const uint64_t* src_offsets, uint8_t* dst,
                             const uint64_t* dst_offsets, uint64_t* sizes, uint32_t* status) {
    if (nblocks == 0) return OXH_OK;
    int rc = snappy_compress_args(nblocks, src, src_offsets, dst_offsets, sizes, status);
    if (rc) return rc;
    SnappyPlan plan;
    if ((rc = snappy_plan(nblocks, src_offsets, dst_offsets, plan))) return rc;
    const uint64_t nfrags = plan.frag_block.size();
    // the bytes the good blocks name, in one piece
    uint64_t lo = UINT64_MAX, hi = 0, ngood = 0;
    for (uint64_t b = 0; b < nblocks; ++b)
        if (plan.good[b]) lo = std::min(lo, src_offsets[b]), hi = std::max(hi, src_offsets[b + 1]), ++ngood;
    if (!ngood) lo = hi = 0;
    if (ngood && !dst) return fail(OXH_ERR_INVALID, "snappy compress: dst is NULL");
    if ((rc = snappy_compress_enter(ctx))) return rc;
    hipStream_t st = ctx->stream;
    // one device block: the input, four offset tables from 0, the sizes, the statuses, then the call's working memory
    const uint64_t up16 = 15, at_tables = (hi - lo + up16) & ~up16, at_sizes = at_tables + 4 * nblocks * 8, at_status = at_sizes + nblocks * 8;
    const SnappyLayout lay(at_status + nblocks * 4, nblocks, nfrags);
    std::vector<uint64_t> tables, got_sizes;
    std::vector<uint32_t> frag_size, got_status;
    try {
        tables.assign(4 * nblocks, 0), got_sizes.resize(nblocks), frag_size.resize(nfrags), got_status.resize(nblocks);
    } catch (const std::bad_alloc&) {
        return fail(OXH_ERR_NOMEM, "snappy compress: the offset tables on the host");
    }
    for (uint64_t b = 0; b < nblocks; ++b)
        if (plan.good[b]) tables[b] = src_offsets[b] - lo, tables[nblocks + b] = src_offsets[b + 1] - lo;
    uint8_t *d = nullptr, *d_out = nullptr;
    if (hipMalloc(&d, lay.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "snappy compress: " + std::to_string(lay.total) + " B for the blocks on the device");
    }
    oxh::poison_device(d, lay.total, st);
    rc = [&]() -> int {
        if (hi > lo) HIP_TRY(hipMemcpyAsync(d, src + lo, hi - lo, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d + at_tables, tables.data(), 2 * nblocks * 8, hipMemcpyHostToDevice, st));
        const uint64_t *d_lo = (const uint64_t*)(d + at_tables), *d_hi = d_lo + nblocks, *d_dlo = d_hi + nblocks, *d_dhi = d_dlo + nblocks;
        int r = snappy_run_fragments(plan, lay, d, d, d_lo, d_hi, st);
        if (r) return r;
        unsigned long long ctrl = 0;
        if (nfrags) HIP_TRY(hipMemcpyAsync(frag_size.data(), d + lay.at_size, nfrags * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&ctrl, d + lay.at_ctrl, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((r = snappy_ctrl_error(ctrl))) return r;
        // the streams' sizes are known: they are packed one behind the other and come down block by block
        uint64_t packed = 0;
        for (uint64_t b = 0; b < nblocks; ++b) {
            tables[2 * nblocks + b] = packed;
            if (plan.good[b]) {
                uint64_t n = src_offsets[b + 1] - src_offsets[b];
                do ++packed; while (n >>= 7);
                for (uint64_t f = plan.frag0[b]; f < plan.frag0[b + 1]; ++f) packed += frag_size[f];
            }
            tables[3 * nblocks + b] = packed;
        }
        if (hipMalloc(&d_out, std::max<uint64_t>(packed, 1)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "snappy compress: " + std::to_string(packed) + " B for the streams on the device");
        }
        oxh::poison_device(d_out, packed, st);
        HIP_TRY(hipMemcpyAsync(d + at_tables + 2 * nblocks * 8, tables.data() + 2 * nblocks, 2 * nblocks * 8, hipMemcpyHostToDevice, st));
        if ((r = oxh::snappy_pack_enqueue(d_lo, d_hi, d_out, d_dlo, d_dhi, (uint64_t*)(d + at_sizes), (uint32_t*)(d + at_status), nblocks, false,
                                          lay.work(d, nfrags), st)))
            return r;
        HIP_TRY(hipMemcpyAsync(got_sizes.data(), d + at_sizes, nblocks * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(got_status.data(), d + at_status, nblocks * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&ctrl, d + lay.at_ctrl, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((r = snappy_ctrl_error(ctrl))) return r;
        for (uint64_t b = 0; b < nblocks; ++b)
            if (plan.good[b] && (got_status[b] || got_sizes[b] != tables[3 * nblocks + b] - tables[2 * nblocks + b])) return snappy_ctrl_error(1);
        // the packed streams come down in one copy and go to their ranges from there
        std::vector<uint8_t> streams;
        try {
            streams.resize(packed);
        } catch (const std::bad_alloc&) {
            return fail(OXH_ERR_NOMEM, "snappy compress: " + std::to_string(packed) + " B for the streams on the host");
        }
        if (packed) HIP_TRY(hipMemcpy(streams.data(), d_out, packed, hipMemcpyDeviceToHost));
        for (uint64_t b = 0; b < nblocks; ++b)
            if (plan.good[b]) memcpy(dst + dst_offsets[b], streams.data() + tables[2 * nblocks + b], got_sizes[b]);
        for (uint64_t b = 0; b < nblocks; ++b) sizes[b] = plan.good[b] ? got_sizes[b] : 0, status[b] = plan.good[b] ? 0 : OXH_SNAPPY_RANGE;
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

int oxh_format_hex(uint64_t lo, uint64_t hi, char* out) {
    if (!out) return 0;
    unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
    char tmp[33];
    int n = 0;
    do {
        tmp[n++] = "0123456789abcdef"[(int)(v & 15)];
        v >>= 4;
    } while (v);
    for (int i = 0; i < n; ++i) out[i] = tmp[n - 1 - i];
    out[n] = 0;
    return n;
}

int oxh_format_dec(uint64_t lo, uint64_t hi, char* out) {
    if (!out) return 0;
    unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
    char tmp[40];
    int n = 0;
    do {
        tmp[n++] = (char)('0' + (int)(v % 10));
        v /= 10;
    } while (v);
    for (int i = 0; i < n; ++i) out[i] = tmp[n - 1 - i];
    out[n] = 0;
    return n;
}

}  // extern "C"
