// oxen_amd/csrc/row_hash.hip -- row hashes of a data frame straight from its columns (oxh_row_hashes_*)
// and the row set-diff of two such digest tables (oxh_row_diff_*): `oxen diff` / `oxen df` on tabular
// files. The reference walks both frames row by row (core/df/tabular.rs:816-945 df_hash_rows /
// df_hash_rows_on_cols: any_val_to_bytes (:651-675) of every cell appended to a Vec<u8>, hash_buffer of
// it), then builds two HashMap<String, u32> over the hex strings (repositories/diffs.rs:1023-1074
// compute_new_row_indices). Here a frame stays columnar (Arrow: values, offsets, validity bitmaps) and a
// row's buffer exists only as the image a lane assembles in LDS (DESIGN.md §4 "Row hashes").
//
// A row's bytes: over the columns in the order given, nothing for a null cell, the raw little-endian
// bytes of a fixed-width cell, one byte 0/1 of a boolean, the bytes of a string / binary cell. Cells are
// not delimited (the reference's behaviour). The digest is XXH3-128, seed 0, of those bytes.
//
// One call is, on one stream:
//   length    one lane per row sums its cell lengths; the largest length, the number of rows above
//             240 B and their bytes are reduced to three words the host reads (it sizes the LDS slots
//             and the long rows' arena from them);
//   short     rows of at most 240 B, one lane per row: the lane copies its cells into its own LDS slot
//             (slots an odd number of dwords apart, so a wave's 64 lanes fall on different banks) and runs
//             xxh3_lane_short over the image. Fixed-width and boolean columns are read with row = lane
//             (coalesced); a wave's 64 string spans are contiguous in the column's bytes;
//   long      rows above 240 B (cells with captions, prompts, JSON): plan (each gets a place in an arena
//             leased from scratch.hpp: a prefix sum of the lengths inside the workgroup, one atomic add
//             per workgroup), gather (one wave per row copies its cells there), K1 for packed items over
//             the arena, scatter of the digests to their rows. There is no second long-path hash.
// No lane waits for another. Offsets that decrease or are negative give a cell of length 0 and set the
// error word (the call then returns OXH_ERR_INVALID): nothing outside the range the offsets name is read.
//
// The diff restates compute_new_row_indices: HashMap::from_iter keeps the LAST row index of each distinct
// hash; `added` is that index for every distinct head digest absent from base, `removed` the mirror image.
// One insert of base then head into a private dedup index (oxh_dedup_index_*, sized for the rows) gives
// every digest an id, its first ordinal; mark takes, per id and side, the largest row index (atomic max),
// flag sets a row's byte when it is that index and the other side has none for the id.
#include "capi_internal.hpp"
#include "columns.hpp"

using namespace oxh::capi;

namespace oxh {

constexpr uint32_t kRowShortMax = 240;  // the XXH3 short paths (xxh3_lane_short)
constexpr unsigned long long kRowErrPlan = 4;  // beside kRowErrOffsets, kRowErrValues (columns.hpp)
// ctrl words of one call
constexpr int kCtrlMax = 0, kCtrlLong = 1, kCtrlLongBytes = 2, kCtrlErr = 3, kCtrlCursor = 4 /* and 5 */, kCtrlWords = 8;

// The kernels below are written once for the two images of columns.hpp (image_cell): KEYED = false hashes
// the reference's row bytes, KEYED = true the grouping's key image (group_rows.hip), whose lengths count the
// tags and the length prefixes.
template <bool KEYED>
__device__ __forceinline__ uint64_t row_length(const RowCol* __restrict__ cols, uint32_t ncols, uint64_t r, unsigned long long& bad) {
    uint64_t len = 0;
    ImageCell cell;
    for (uint32_t k = 0; k < ncols; ++k) len += image_cell<KEYED>(cols[k], r, cell, bad);
    return len;
}

// ctrl[kCtrlMax] = the largest row length, ctrl[kCtrlLong] / [kCtrlLongBytes] = the rows above short_max
// and their bytes. Grid-stride, so the reduction costs a few thousand atomics whatever nrows is.
template <bool KEYED>
__global__ __launch_bounds__(256) void row_length_kernel(const RowCol* __restrict__ cols, uint32_t ncols, uint64_t nrows,
                                                         uint32_t short_max, unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long part[4][3];
    uint64_t most = 0, nlong = 0, lbytes = 0;
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += stride) {
        const uint64_t len = row_length<KEYED>(cols, ncols, r, bad);
        most = len > most ? len : most;
        if (len > short_max) {
            nlong += 1;
            lbytes += len;
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every lane is here (nothing above returns)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t m = (uint64_t)__shfl_xor((long long)most, off, 64);
        most = m > most ? m : most;
        nlong += (uint64_t)__shfl_xor((long long)nlong, off, 64);
        lbytes += (uint64_t)__shfl_xor((long long)lbytes, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* mine = part[threadIdx.x >> 6];
        mine[0] = most, mine[1] = nlong, mine[2] = lbytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0, n = 0, b = 0;
        for (int w = 0; w < 4; ++w) {
            m = part[w][0] > m ? part[w][0] : m;
            n += part[w][1];
            b += part[w][2];
        }
        if (m) atomicMax(&ctrl[kCtrlMax], m);
        if (n) {
            atomicAdd(&ctrl[kCtrlLong], n);
            atomicAdd(&ctrl[kCtrlLongBytes], b);
        }
    }
}

// Rows [row0, nrows) of at most `cap` bytes, one lane per row; `stride` (bytes, an odd number of dwords,
// at least cap) apart in dynamic LDS. A row above cap is a long row and is left to the long path.
template <bool KEYED>
__global__ __launch_bounds__(256) void row_hash_short_kernel(const RowCol* __restrict__ cols, uint32_t ncols, uint64_t row0,
                                                             uint64_t nrows, uint32_t stride, uint32_t cap,
                                                             uint64_t* __restrict__ out,
                                                             unsigned long long* __restrict__ ctrl) {
    extern __shared__ uint32_t row_image[];
    const uint64_t r = row0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;  // no barrier and no shuffle below
    uint8_t* slot = (uint8_t*)row_image + threadIdx.x * stride;
    uint32_t pos = 0;
    unsigned long long bad = 0;
    for (uint32_t k = 0; k < ncols; ++k) {
        const RowCol c = cols[k];
        ImageCell cell;
        const uint64_t len = image_cell<KEYED>(c, r, cell, bad);
        if (len > cap - pos) return;  // a long row (pos <= cap always)
        image_put_lane<KEYED>(slot + pos, c, r, cell);
        pos += (uint32_t)len;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const U128 h = xxh3_lane_short(slot, pos);
    out[2 * r] = h.lo;
    out[2 * r + 1] = h.hi;
}

// Every row above short_max gets an index in the long-row lists and a place in the arena: an exclusive
// prefix sum of (1, length) over the workgroup's rows -- ballot and shuffles in the wave, the four wave
// totals through LDS -- on top of what one atomic add per workgroup and counter returns. Which workgroup
// comes first is not fixed; the digests are scattered back by row, so the result is.
template <bool KEYED>
__global__ __launch_bounds__(256) void row_long_plan_kernel(const RowCol* __restrict__ cols, uint32_t ncols, uint64_t row0,
                                                            uint64_t nrows, uint32_t short_max, uint64_t cap_rows,
                                                            uint64_t cap_bytes, uint64_t* __restrict__ long_row,
                                                            uint64_t* __restrict__ long_off, uint64_t* __restrict__ long_len,
                                                            unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long wave_sum[4][2], wave_base[4][2];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r = row0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = 0;
    const uint64_t len = r < nrows ? row_length<KEYED>(cols, ncols, r, bad) : 0;  // the error word was set by the length pass
    const bool is_long = len > short_max;
    const unsigned long long who = __ballot(is_long);
    const uint64_t rank = __popcll(who & ((1ull << lane) - 1));
    uint64_t incl = is_long ? len : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((long long)incl, off, 64);
        if (lane >= (unsigned)off) incl += up;
    }
    if (lane == 63) wave_sum[wave][0] = __popcll(who), wave_sum[wave][1] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long n = 0, b = 0;
        for (int w = 0; w < 4; ++w) {
            wave_base[w][0] = n, wave_base[w][1] = b;
            n += wave_sum[w][0], b += wave_sum[w][1];
        }
        const unsigned long long n0 = n ? atomicAdd(&ctrl[kCtrlCursor], n) : 0;
        const unsigned long long b0 = n ? atomicAdd(&ctrl[kCtrlCursor + 1], b) : 0;
        for (int w = 0; w < 4; ++w) wave_base[w][0] += n0, wave_base[w][1] += b0;
    }
    __syncthreads();
    if (!is_long) return;
    const uint64_t idx = wave_base[wave][0] + rank, off = wave_base[wave][1] + (incl - len);
    if (idx >= cap_rows || off > cap_bytes || len > cap_bytes - off) {  // not what the length pass counted
        __hip_atomic_fetch_or(&ctrl[kCtrlErr], kRowErrPlan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    long_row[idx] = r;
    long_off[idx] = off;
    long_len[idx] = len;
}

// One wave per long row: its cells, 8 bytes per lane and step, to arena[long_off .. + long_len).
// (The lists were zeroed: an entry the plan did not fill is row 0 with length 0 and copies nothing.)
template <bool KEYED>
__global__ __launch_bounds__(256) void row_long_gather_kernel(const RowCol* __restrict__ cols, uint32_t ncols, uint64_t nlong,
                                                              const uint64_t* __restrict__ long_row,
                                                              const uint64_t* __restrict__ long_off,
                                                              const uint64_t* __restrict__ long_len, uint8_t* __restrict__ arena) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nlong) return;  // the whole wave
    const uint64_t r = long_row[w], limit = long_len[w];
    uint8_t* dst = arena + long_off[w];
    uint64_t pos = 0;
    unsigned long long bad = 0;
    for (uint32_t k = 0; k < ncols; ++k) {
        const RowCol c = cols[k];
        ImageCell cell;
        const uint64_t n = image_cell<KEYED>(c, r, cell, bad);
        if (n > limit - pos) return;  // never past the row's place (pos <= limit always)
        image_put_wave<KEYED>(dst + pos, c, r, cell, lane);
        pos += n;
    }
}

__global__ __launch_bounds__(256) void row_long_scatter_kernel(const uint64_t* __restrict__ long_row,
                                                               const uint64_t* __restrict__ digests, uint64_t nlong,
                                                               uint64_t nrows, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlong) return;
    const uint64_t r = long_row[i];
    if (r >= nrows) return;
    out[2 * r] = digests[2 * i];
    out[2 * r + 1] = digests[2 * i + 1];
}

// ---------------------------------------------------------------- row diff
constexpr unsigned long long kDiffErrFirst = 1;

// Rows [0, nbase) are base, [nbase, n) head; first[i] = the id of row i's digest (the smallest ordinal that
// carries it). last[2 * id + side] = 1 + the largest row index of that side with the id (0: none).
__global__ __launch_bounds__(256) void row_diff_mark_kernel(const uint64_t* __restrict__ first, uint64_t nbase, uint64_t n,
                                                            unsigned int* __restrict__ last,
                                                            unsigned long long* __restrict__ ctrl) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t id = first[i];
        if (id >= n) {  // not an ordinal of this call: never index `last` with it
            __hip_atomic_fetch_or(&ctrl[2], kDiffErrFirst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const unsigned side = i >= nbase;
        const unsigned int mine = (unsigned int)(side ? i - nbase : i) + 1;
        unsigned int* p = &last[2 * id + side];
        // a hint, as in the index's insert: values only rise, so one seen at or above mine stays there
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine)
            __hip_atomic_fetch_max(p, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// (every max of the mark has landed) flag[row] = 1 when the row is the last of its digest on its side and
// the other side has none; ctrl[0] / ctrl[1] += the flagged rows of base / head, summed per wave (ballot)
// and workgroup first.
__global__ __launch_bounds__(256) void row_diff_flag_kernel(const uint64_t* __restrict__ first, uint64_t nbase, uint64_t n,
                                                            const unsigned int* __restrict__ last, uint8_t* __restrict__ removed,
                                                            uint8_t* __restrict__ added, unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long part[4][2];
    unsigned long long cnt[2] = {0, 0};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const bool live = i < n;
        const unsigned side = live && i >= nbase;
        bool flag = false;
        if (live) {
            const uint64_t id = first[i], local = side ? i - nbase : i;
            if (id < n) flag = last[2 * id + side] == (unsigned int)local + 1 && last[2 * id + (side ^ 1)] == 0;
            (side ? added : removed)[local] = flag ? 1 : 0;
        }
        cnt[0] += __popcll(__ballot(flag && !side));
        cnt[1] += __popcll(__ballot(flag && side));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][0] = cnt[0], part[threadIdx.x >> 6][1] = cnt[1];
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (sum) atomicAdd(&ctrl[threadIdx.x], sum);
    }
}

}  // namespace oxh

namespace {

constexpr uint64_t kMaxHashRows = 1ull << 40;
constexpr uint64_t kMaxDiffRows = 0xFFFFFFFFull;   // the reference's Vec<u32>
constexpr uint64_t kLaunchRows = 1ull << 38;       // rows of one row-per-lane launch: the grid fits 31 bits
constexpr int kVariantGatherAll = 9001;            // oxh_set_kernel_variant: every row through the arena (tools/row_hash_probe.py)

using oxh::cols::is_bytes;
using oxh::cols::known_kind;
unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }
unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 2048); }  // as the index's resolve

// What both row-hash forms check before they need a device. `done`: nrows == 0, nothing to do.
int row_arguments(uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* values, const void* const* offsets,
                  const uint8_t* const* validity, const uint64_t* bit_offsets, const uint64_t* out, bool host, bool& done) {
    done = false;
    if (!kinds || !values || !offsets || !validity || !bit_offsets)
        return fail(OXH_ERR_INVALID, "row hashes: kinds, values, offsets, validity or bit_offsets is NULL");
    if (ncols == 0) return fail(OXH_ERR_INVALID, "row hashes: ncols is 0");
    for (uint32_t c = 0; c < ncols; ++c)
        if (!known_kind(kinds[c]))
            return fail(OXH_ERR_INVALID, "row hashes: column " + std::to_string(c) + " has unknown kind " + std::to_string(kinds[c]));
    if (nrows > kMaxHashRows) return fail(OXH_ERR_INVALID, "row hashes: more than 2^40 rows");
    if (nrows == 0) {
        done = true;
        return OXH_OK;
    }
    for (uint32_t c = 0; c < ncols; ++c) {
        const std::string what = oxh::cols::column_error("row hashes: column " + std::to_string(c), kinds[c], values[c], offsets[c],
                                                         nrows, host);
        if (!what.empty()) return fail(OXH_ERR_INVALID, what);
    }
    if (!out) return fail(OXH_ERR_INVALID, "row hashes: out is NULL");
    return OXH_OK;
}

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

int row_error(unsigned long long e, bool keyed = false) {
    if (!e) return OXH_OK;
    const std::string who = keyed ? "group rows" : "row hashes";
    if (e & oxh::kRowErrPlan) return fail(OXH_ERR_HIP, who + ": the long rows changed between the length pass and the plan");
    if (e & oxh::kRowErrOffsets) return fail(OXH_ERR_INVALID, who + ": a byte column's offsets decrease or are negative");
    return fail(OXH_ERR_INVALID, who + ": a byte column has bytes but no values");
}

// The three steps over device-resident columns; complete on return.
int row_hashes_run(uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                   const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets, uint64_t* d_out,
                   hipStream_t st) {
    RowImageCall call;
    int rc = call.measure(false, nrows, ncols, kinds, nullptr, d_values, d_offsets, d_validity, bit_offsets, st);
    if (rc) return rc;
    if (!call.nlong) return call.hash(d_out, nullptr, st);
    oxh::ScratchLease lease(st);  // ends (and waits for the stream) before the call's block is freed
    void* base = nullptr;
    if (lease.get(call.scratch_bytes(), &base) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        return fail(OXH_ERR_NOMEM, "row hashes: arena of " + std::to_string(call.long_bytes) + " B for " + std::to_string(call.nlong) + " long rows");
    }
    return call.hash(d_out, base, st);
}

// ---------------------------------------------------------------- row diff
int diff_arguments(const uint64_t* base, uint64_t nbase, const uint64_t* head, uint64_t nhead, const void* removed,
                   const void* added, uint64_t* counts2, bool& done) {
    done = false;
    if (!counts2) return fail(OXH_ERR_INVALID, "row diff: counts2 is NULL");
    if (nbase > kMaxDiffRows || nhead > kMaxDiffRows) return fail(OXH_ERR_INVALID, "row diff: more than 2^32 - 1 rows");
    if ((nbase && !base) || (nhead && !head)) return fail(OXH_ERR_INVALID, "row diff: a digest table is NULL");
    if ((nbase && !removed) || (nhead && !added)) return fail(OXH_ERR_INVALID, "row diff: an output is NULL");
    if (nbase + nhead == 0) {
        counts2[0] = counts2[1] = 0;
        done = true;
    }
    return OXH_OK;
}

// base then head (device tables) through a private index; flags to d_removed / d_added, complete on return
int row_diff_run(oxh_ctx* ctx, const uint64_t* d_base, uint64_t nbase, const uint64_t* d_head, uint64_t nhead,
                 uint8_t* d_removed, uint8_t* d_added, uint64_t* counts2, hipStream_t st) {
    const uint64_t n = nbase + nhead;
    // everything is made before any work starts: [first n u64 | ctrl 4 u64 | last 2n u32]
    void* index = nullptr;
    uint64_t* d_block = nullptr;
    unsigned long long* h_ctrl = nullptr;
    auto release = [&](int rc) {
        if (rc != OXH_OK) (void)hipStreamSynchronize(st);  // work of a failed call may still be queued
        if (d_block) (void)hipFree(d_block);
        if (h_ctrl) (void)hipHostFree(h_ctrl);
        if (index) (void)oxh_dedup_index_destroy(index);
        return rc;
    };
    int rc = oxh_dedup_index_create(ctx, n, &index);
    if (rc) return release(rc);
    if (hipMalloc(&d_block, (n + 4) * 8 + 2 * n * 4) != hipSuccess || hipHostMalloc(&h_ctrl, 4 * 8, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return release(fail(OXH_ERR_NOMEM, "row diff: " + std::to_string(n) + " rows of ids and last indices"));
    }
    oxh::poison_device(d_block, (n + 4) * 8 + 2 * n * 4, st), oxh::poison_pinned(h_ctrl, 4 * 8);
    uint64_t* d_first = d_block;
    unsigned long long* d_ctrl = (unsigned long long*)(d_block + n);
    unsigned int* d_last = (unsigned int*)(d_ctrl + 4);
    rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, 4 * 8 + 2 * n * 4, st));
        int r = OXH_OK;
        if (nbase && (r = oxh_dedup_index_insert_device(index, d_base, nullptr, nbase, d_first, nullptr, st))) return r;
        if (nhead && (r = oxh_dedup_index_insert_device(index, d_head, nullptr, nhead, d_first + nbase, nullptr, st))) return r;
        oxh::row_diff_mark_kernel<<<stride_grid(n), 256, 0, st>>>(d_first, nbase, n, d_last, d_ctrl);
        HIP_TRY(hipGetLastError());
        oxh::row_diff_flag_kernel<<<stride_grid(n), 256, 0, st>>>(d_first, nbase, n, d_last, d_removed, d_added, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 4 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_ctrl[2]) return fail(OXH_ERR_HIP, "row diff: a first ordinal is not below the row count; no result");
        counts2[0] = h_ctrl[0];
        counts2[1] = h_ctrl[1];
        return OXH_OK;
    }();
    return release(rc);
}

}  // namespace

namespace oxh::capi {

int RowImageCall::measure(bool keyed_image, uint64_t rows, uint32_t cols, const uint32_t* kinds, const uint32_t* orders,
                          const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                          const uint64_t* bit_offsets, hipStream_t st) {
    using oxh::RowCol;
    keyed = keyed_image, nrows = rows, ncols = cols;
    gather_all = g_variant.load() == kVariantGatherAll;
    short_max = gather_all ? 0 : oxh::kRowShortMax;
    ctrl_at = (ncols * sizeof(RowCol) + 63) & ~(size_t)63;
    const size_t bytes = ctrl_at + oxh::kCtrlWords * 8;
    int rc = block.make(bytes, keyed ? "group rows" : "row hashes", st);
    if (rc) return rc;
    RowCol* h_cols = (RowCol*)block.h;
    for (uint32_t c = 0; c < ncols; ++c) {
        h_cols[c].values = (const uint8_t*)d_values[c];
        h_cols[c].offsets = is_bytes(kinds[c]) ? (const uint8_t*)d_offsets[c] : nullptr;
        h_cols[c].validity = d_validity[c];
        h_cols[c].vbit = bit_offsets[2 * c];
        h_cols[c].nbit = bit_offsets[2 * c + 1];
        h_cols[c].kind = kinds[c];
        h_cols[c].order = orders ? orders[c] : 0;
    }
    const RowCol* d_cols = (const RowCol*)block.d;
    unsigned long long* d_ctrl = (unsigned long long*)(block.d + ctrl_at);
    const unsigned long long* h_ctrl = (const unsigned long long*)(block.h + ctrl_at);
    HIP_TRY(hipMemcpyAsync(block.d, block.h, bytes, hipMemcpyHostToDevice, st));
    if (keyed)
        oxh::row_length_kernel<true><<<stride_grid(nrows), 256, 0, st>>>(d_cols, ncols, nrows, short_max, d_ctrl);
    else
        oxh::row_length_kernel<false><<<stride_grid(nrows), 256, 0, st>>>(d_cols, ncols, nrows, short_max, d_ctrl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(block.h + ctrl_at, d_ctrl, oxh::kCtrlWords * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = row_error(h_ctrl[oxh::kCtrlErr], keyed))) {
        if (!keyed) return rc;
        deferred = rc;  // the bad cells are empty cells: the call finishes and says so at the end
    }
    longest = h_ctrl[oxh::kCtrlMax], nlong = h_ctrl[oxh::kCtrlLong], long_bytes = h_ctrl[oxh::kCtrlLongBytes];
    STEP("%s: %llu rows, longest %llu B, %llu long rows of %llu B", keyed ? "group rows" : "row hashes", (unsigned long long)nrows,
         (unsigned long long)longest, (unsigned long long)nlong, (unsigned long long)long_bytes);
    return OXH_OK;
}

// [long_row | long_off | long_len | digests 2 | arena]
uint64_t RowImageCall::scratch_bytes() const { return nlong ? ((5 * nlong * 8 + 255) & ~255ull) + long_bytes + 256 : 0; }

int RowImageCall::hash(uint64_t* d_out, void* scratch, hipStream_t st) {
    using oxh::RowCol;
    const RowCol* d_cols = (const RowCol*)block.d;
    unsigned long long* d_ctrl = (unsigned long long*)(block.d + ctrl_at);
    const unsigned long long* h_ctrl = (const unsigned long long*)(block.h + ctrl_at);
    if (nlong < nrows) {
        // slots as long as the longest short row can be, an odd number of dwords apart: the 64 lanes of a
        // wave on different banks, and more workgroups per CU on the common 30-100 B rows than 244 B gives
        const uint32_t cap = (uint32_t)std::min<uint64_t>(longest, short_max);
        const uint32_t stride = 4 * (std::max<uint32_t>(1, (cap + 3) / 4) | 1);
        for (uint64_t at = 0; at < nrows; at += kLaunchRows) {
            const uint64_t end = std::min(nrows, at + kLaunchRows);
            if (keyed)
                oxh::row_hash_short_kernel<true><<<grid_for(end - at), 256, 256 * stride, st>>>(d_cols, ncols, at, end, stride, cap, d_out, d_ctrl);
            else
                oxh::row_hash_short_kernel<false><<<grid_for(end - at), 256, 256 * stride, st>>>(d_cols, ncols, at, end, stride, cap, d_out, d_ctrl);
            HIP_TRY(hipGetLastError());
        }
    }
    if (nlong) {
        // the lists zeroed
        void* base = scratch;
        const uint64_t lists = 5 * nlong * 8, arena_at = (lists + 255) & ~255ull;
        uint64_t *long_row = (uint64_t*)base, *long_off = long_row + nlong, *long_len = long_off + nlong, *dig = long_len + nlong;
        uint8_t* arena = (uint8_t*)base + arena_at;
        HIP_TRY(hipMemsetAsync(base, 0, 3 * nlong * 8, st));
        for (uint64_t at = 0; at < nrows; at += kLaunchRows) {
            const uint64_t end = std::min(nrows, at + kLaunchRows);
            if (keyed)
                oxh::row_long_plan_kernel<true><<<grid_for(end - at), 256, 0, st>>>(d_cols, ncols, at, end, short_max, nlong, long_bytes,
                                                                                   long_row, long_off, long_len, d_ctrl);
            else
                oxh::row_long_plan_kernel<false><<<grid_for(end - at), 256, 0, st>>>(d_cols, ncols, at, end, short_max, nlong, long_bytes,
                                                                                    long_row, long_off, long_len, d_ctrl);
            HIP_TRY(hipGetLastError());
        }
        if (keyed)
            oxh::row_long_gather_kernel<true><<<(unsigned)((nlong + 3) / 4), 256, 0, st>>>(d_cols, ncols, nlong, long_row, long_off, long_len, arena);
        else
            oxh::row_long_gather_kernel<false><<<(unsigned)((nlong + 3) / 4), 256, 0, st>>>(d_cols, ncols, nlong, long_row, long_off, long_len, arena);
        HIP_TRY(hipGetLastError());
        int rc = gather_all ? launch_lane(arena, long_off, long_len, nlong, dig, st)
                            : launch_wave(arena, long_off, long_len, nlong, dig, st, ItemShape::Packed);
        if (rc) return rc;
        oxh::row_long_scatter_kernel<<<grid_for(nlong), 256, 0, st>>>(long_row, dig, nlong, nrows, d_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(block.h + ctrl_at, d_ctrl, oxh::kCtrlWords * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // before a lease ends
    const int rc = row_error(h_ctrl[oxh::kCtrlErr], keyed);
    if (keyed && (rc == OXH_OK || rc == OXH_ERR_INVALID)) return OXH_OK;  // `deferred` says it
    return rc;
}

}  // namespace oxh::capi

extern "C" {

int oxh_row_hashes_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                          const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                          uint64_t* d_out, void* stream) {
    bool done = false;
    int rc = row_arguments(nrows, ncols, kinds, d_values, d_offsets, d_validity, bit_offsets, d_out, false, done);
    if (rc || done) return rc;
    if ((rc = device_enter(ctx))) return rc;
    return row_hashes_run(nrows, ncols, kinds, d_values, d_offsets, d_validity, bit_offsets, d_out, (hipStream_t)stream);
}

int oxh_row_hashes_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* values,
                        const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets, uint64_t* out) {
    bool done = false;
    int rc = row_arguments(nrows, ncols, kinds, values, offsets, validity, bit_offsets, out, true, done);
    if (rc || done) return rc;
    if ((rc = device_enter(ctx))) return rc;
    hipStream_t st = ctx->stream;
    // One device block: the digests, then for every column only what its rows name -- nrows values (the
    // bytes that hold its bits for a boolean), the nrows + 1 offsets and the span [offsets[0],
    // offsets[nrows]) of a byte column, the bytes that hold its validity bits -- each 16-B aligned.
    oxh::cols::Staging plan;
    plan.total = nrows * 16;
    std::vector<oxh::cols::Staged> staged(ncols);
    std::vector<const void*> d_values(ncols, nullptr), d_offsets(ncols, nullptr);
    std::vector<const uint8_t*> d_validity(ncols, nullptr);
    std::vector<uint64_t> bits(2 * (size_t)ncols, 0);
    for (uint32_t c = 0; c < ncols; ++c)
        staged[c] = plan.add_column(kinds[c], values[c], offsets[c], validity[c], bit_offsets[2 * c], bit_offsets[2 * c + 1], nrows);
    const uint64_t total = plan.total;
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "row hashes: " + std::to_string(total) + " B for the columns on the device");
    }
    oxh::poison_device(d_block, total, st);
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : plan.pieces) HIP_TRY(hipMemcpyAsync(d_block + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        for (uint32_t c = 0; c < ncols; ++c) {
            d_values[c] = plan.values_at(d_block, staged[c]);
            d_offsets[c] = plan.offsets_at(d_block, staged[c]);
            d_validity[c] = plan.validity_at(d_block, staged[c]);
            bits[2 * c] = staged[c].vbit, bits[2 * c + 1] = staged[c].nbit;
        }
        int r = row_hashes_run(nrows, ncols, kinds, d_values.data(), d_offsets.data(), d_validity.data(), bits.data(),
                               (uint64_t*)d_block, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(out, d_block, nrows * 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    return rc;
}

int oxh_row_diff_device(oxh_ctx* ctx, const uint64_t* d_base, uint64_t nbase, const uint64_t* d_head, uint64_t nhead,
                        uint8_t* d_removed, uint8_t* d_added, uint64_t* counts2, void* stream) {
    bool done = false;
    int rc = diff_arguments(d_base, nbase, d_head, nhead, d_removed, d_added, counts2, done);
    if (rc || done) return rc;
    if ((rc = device_enter(ctx))) return rc;
    return row_diff_run(ctx, d_base, nbase, d_head, nhead, d_removed, d_added, counts2, (hipStream_t)stream);
}

int oxh_row_diff_host(oxh_ctx* ctx, const uint64_t* base, uint64_t nbase, const uint64_t* head, uint64_t nhead,
                      uint32_t* removed_idx, uint32_t* added_idx, uint64_t* counts2) {
    bool done = false;
    int rc = diff_arguments(base, nbase, head, nhead, removed_idx, added_idx, counts2, done);
    if (rc || done) return rc;
    if ((rc = device_enter(ctx))) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n = nbase + nhead;
    // [digests 2n u64 | flags n bytes] on the device, the flags back into a host vector
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, n * 17) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "row diff: " + std::to_string(n) + " rows of digests on the device");
    }
    oxh::poison_device(d_block, n * 17, st);
    std::vector<uint8_t> flags;
    uint64_t counts[2] = {0, 0};
    rc = [&]() -> int {
        flags.resize(n);
        uint64_t* d_dig = (uint64_t*)d_block;
        uint8_t* d_flags = d_block + n * 16;
        if (nbase) HIP_TRY(hipMemcpyAsync(d_dig, base, nbase * 16, hipMemcpyHostToDevice, st));
        if (nhead) HIP_TRY(hipMemcpyAsync(d_dig + 2 * nbase, head, nhead * 16, hipMemcpyHostToDevice, st));
        int r = row_diff_run(ctx, d_dig, nbase, d_dig + 2 * nbase, nhead, d_flags, d_flags + nbase, counts, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(flags.data(), d_flags, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    if (rc) return rc;
    uint64_t k = 0;
    for (uint64_t i = 0; i < nbase; ++i)
        if (flags[i]) removed_idx[k++] = (uint32_t)i;
    k = 0;
    for (uint64_t i = 0; i < nhead; ++i)
        if (flags[nbase + i]) added_idx[k++] = (uint32_t)i;
    counts2[0] = counts[0];
    counts2[1] = counts[1];
    return OXH_OK;
}

}  // extern "C"
