// oxen_amd/csrc/filter_rows.hip -- the rows of a frame that a filter selects (oxh_filter_rows_*): `oxen df
// --filter "label == dog && min_x > 0.5"` (core/df/tabular.rs:404-422 filter_df, :391-402 filter_from_val) from
// the columns the terms name (Arrow: values, offsets, validity bitmaps) on the device. The semantics are stated
// in include/oxen_hash.h (DESIGN.md §4 "Filter"); a term, the three-valued && / || and the fold are
// filter_terms.hpp's, the code tests/native/filter_rows_host_test.cpp runs on the host.
//
// One call is, on one stream:
//   evaluate  filter_eval_kernel, one lane per row, grid-stride, every wave on whole 64-row blocks (block k =
//             rows 64k .. 64k+63), four neighbouring blocks side by side: a lane evaluates all terms of its rows
//             and folds them; the ballot of "true" is
//             mask word k, which one lane stores with its popcount beside it (counts[k]); "selected" and "null
//             result" are summed per wave, per workgroup (LDS), then one atomic each. The term descriptors are
//             kernel arguments and the literal bytes sit in LDS: uniform reads, no per-lane gather;
//   scan      exclusive_scan_u32 over counts: ceil(n / 64) entries, not n -- the compaction costs n / 8 bytes
//             of mask and 12 B per block, not a flag and a scanned flag per row;
//   emit      filter_emit_kernel, a later launch: every wave reads its block's mask word and base again, and a
//             lane whose bit is set stores its row at base + the set bits below it.
// Without idx there is no scan and no emit. No lane ever waits for another lane or workgroup; launches order
// the steps. A place from the scan is checked against the selected rows and the row before it is stored
// through: a bad one sets the error word (OXH_ERR_HIP). A bad pair of offsets is a cell of length 0 (row_cell)
// and sets the error word too: the call finishes and returns OXH_ERR_INVALID.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "filter_rows_host.hpp"

using namespace oxh::capi;

namespace oxh {

constexpr unsigned long long kFilterErrPlace = 4;  // beside columns.hpp's kRowErrOffsets and kRowErrValues
// ctrl words of one call: the error word, then stats2
constexpr int kFilterCtrlErr = 0, kFilterCtrlSelected = 1, kFilterCtrlNull = 2, kFilterCtrlWords = 3;
constexpr uint32_t kFilterLitWords = filterrows::kLitBlock / 8;
// 64-row blocks a wave evaluates side by side, and the rows of a workgroup's four waves in one round: one load per
// lane in flight (59 us for 10 M Int64 rows, 1.4 TB/s) does not keep the memory busy
constexpr uint32_t kFilterWaveBlocks = 4, kFilterGroupRows = 256 * kFilterWaveBlocks;

struct FilterTerm {
    RowCol col;
    uint64_t word;              // the literal of a fixed-width term (little-endian bytes, zero-extended); a boolean's 0 / 1
    uint32_t op;                // OXH_FILTER_EQ ..
    uint32_t lit_at, lit_len;   // a byte term's literal in the literal block (lit_at is a multiple of 8)
    uint32_t unused;
};

// The whole filter, passed by value as kernel arguments: the same for every lane of the grid.
struct FilterCall {
    FilterTerm term[OXH_FILTER_MAX_TERMS];
    uint32_t nterms;
    uint32_t or_bits;     // bit t - 1: the operator in front of term t is ||
    uint32_t lit_words;   // 8-byte words of the literal block in use
    uint32_t unused;
};

// Term t on row r: kFalse / kTrue / kNull.
__device__ __forceinline__ uint32_t filter_term(const FilterTerm& t, uint64_t r, const uint8_t* lits, unsigned long long& bad) {
    const RowCol& c = t.col;
    uint64_t start = 0;
    const uint64_t len = row_cell(c, r, start, bad);  // a bad pair of offsets: length 0
    if (c.validity && !row_bit(c.validity, c.nbit + r)) return filterterms::kNull;
    int cmp;
    switch (c.kind) {
        case OXH_COL_FIXED1: cmp = filterterms::compare_fixed(c.order, 1, c.values[r], t.word); break;
        case OXH_COL_FIXED4: cmp = filterterms::compare_fixed(c.order, 4, ld32u(c.values + 4 * r), t.word); break;
        case OXH_COL_FIXED8: cmp = filterterms::compare_fixed(c.order, 8, ld64u(c.values + 8 * r), t.word); break;
        case OXH_COL_BOOL: cmp = filterterms::compare_words(row_bit(c.values, c.vbit + r) ? 1 : 0, t.word); break;
        default: cmp = filterterms::compare_bytes_for(t.op, c.values + start, len, lits + t.lit_at, t.lit_len); break;
    }
    return filterterms::term_result(t.op, cmp);
}

// mask[k] (may be NULL) = the selected rows of block k, counts[k] (may be NULL) = how many; ctrl: the two sums.
__global__ __launch_bounds__(256) void filter_eval_kernel(const FilterCall call, const uint64_t* __restrict__ lit_block, uint64_t n,
                                                          uint64_t* __restrict__ mask, uint32_t* __restrict__ counts,
                                                          unsigned long long* __restrict__ ctrl) {
    __shared__ uint64_t lits[kFilterLitWords];
    __shared__ unsigned long long part[4][2];
    for (uint32_t w = threadIdx.x; w < call.lit_words && w < kFilterLitWords; w += 256) lits[w] = lit_block[w];
    __syncthreads();
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long selected = 0, nulls = 0, bad = 0;  // the sums are the same in every lane of a wave
    const uint64_t stride = (uint64_t)gridDim.x * kFilterGroupRows;  // a multiple of 64: a wave stays on whole blocks
    const uint64_t rounds = (n + stride - 1) / stride;                // uniform: every lane reaches the ballots
    for (uint64_t t = 0; t < rounds; ++t) {
        // the wave's kFilterWaveBlocks neighbouring blocks, term by term: a column's loads for all of them are in flight together
        const uint64_t first = t * stride + (uint64_t)blockIdx.x * kFilterGroupRows + (uint64_t)wave * (64 * kFilterWaveBlocks) + lane;
        uint32_t result[kFilterWaveBlocks];
#pragma unroll
        for (uint32_t u = 0; u < kFilterWaveBlocks; ++u) {
            const uint64_t i = first + 64 * u;
            // a lane past the rows selects nothing: the mask's tail bits are 0
            result[u] = i < n ? filter_term(call.term[0], i, (const uint8_t*)lits, bad) : filterterms::kFalse;
        }
        for (uint32_t k = 1; k < call.nterms; ++k) {
#pragma unroll
            for (uint32_t u = 0; u < kFilterWaveBlocks; ++u) {
                const uint64_t i = first + 64 * u;
                if (i < n) result[u] = filterterms::fold_step(result[u], filter_term(call.term[k], i, (const uint8_t*)lits, bad), k, call.or_bits);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kFilterWaveBlocks; ++u) {
            const uint64_t i = first + 64 * u;
            const unsigned long long word = __ballot(result[u] == filterterms::kTrue);
            selected += __popcll(word);
            nulls += __popcll(__ballot(result[u] == filterterms::kNull));
            if (lane == 0 && i < n) {  // i is the block's first row here
                if (mask) mask[i >> 6] = word;
                if (counts) counts[i >> 6] = (uint32_t)__popcll(word);
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kFilterCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) {
        unsigned long long* mine = part[threadIdx.x >> 6];
        mine[0] = selected, mine[1] = nulls;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (sum) atomicAdd(&ctrl[kFilterCtrlSelected + threadIdx.x], sum);
    }
}

// (the masks are written, the counts scanned, the sums have landed) idx[base of the row's block + the selected
// rows below it in the block] = the row, for every selected row.
__global__ __launch_bounds__(256) void filter_emit_kernel(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ bases, uint64_t n,
                                                          uint32_t* __restrict__ idx, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long selected = ctrl[kFilterCtrlSelected];
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t word = mask[i >> 6];  // one word for the wave
        if (!((word >> lane) & 1)) continue;
        const uint64_t place = bases[i >> 6] + (uint64_t)__popcll(word & ((1ull << lane) - 1));
        if (place < selected && place <= i)  // the selected rows before row i: never a store outside the n places
            idx[place] = (uint32_t)i;
        else
            bad |= kFilterErrPlace;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kFilterCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oxh

namespace {

namespace filterrows = oxh::filterrows;

unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 2048); }
unsigned eval_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + oxh::kFilterGroupRows - 1) / oxh::kFilterGroupRows, 2048); }

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// One call over device-resident columns (only those a term names are looked at); the outputs that were asked
// for are filled and the stream has drained on return. The control words, the literal block, the counts, their
// scan and -- without the caller's -- the mask are one lease (filter_rows_host.hpp's Lease), with the lease's
// pinned block for what goes up and comes back.
int filter_rows_run(const filterrows::Args& a, const void* const* d_values, const void* const* d_offsets,
                    const uint8_t* const* d_validity, const uint64_t* bits, uint32_t* d_idx, uint64_t* d_mask, uint64_t* stats2,
                    hipStream_t st) {
    using namespace oxh;
    const uint64_t n = a.nrows, blocks = filterrows::blocks_of(n);
    const filterrows::Literals lits(a);
    FilterCall call;
    memset(&call, 0, sizeof call);
    call.nterms = a.nterms;
    call.or_bits = filterrows::or_bits_of(a);
    call.lit_words = (uint32_t)(lits.bytes.size() / 8);
    if (call.lit_words > kFilterLitWords) return fail(OXH_ERR_HIP, "filter rows: the literals outgrow their block");
    for (uint32_t t = 0; t < a.nterms; ++t) {
        const uint32_t c = a.term_col[t], kind = a.kinds[c];
        FilterTerm& term = call.term[t];
        term.col = RowCol{(const uint8_t*)d_values[c], (const uint8_t*)d_offsets[c], d_validity[c], bits[2 * c], bits[2 * c + 1], kind, a.orders[c]};
        term.op = a.term_op[t];
        term.word = a.term_word[t];
        term.lit_at = lits.at[t], term.lit_len = lits.len[t];
    }
    if (d_idx && filterrows::scan_tiles_of(blocks) != scan_tiles(blocks)) return fail(OXH_ERR_HIP, "filter rows: the scan's tile is not the lease's");
    // Everything the call needs beside the columns is one lease: nothing is allocated once a call has run.
    const filterrows::Lease at(n, d_idx != nullptr, d_mask == nullptr);
    ScratchLease lease(st);  // ends (and waits for the stream) when the call returns
    void* base = nullptr;
    void* pinned = nullptr;  // the literal block as it goes up, then the control words as they come back
    if (lease.get(at.total, &base) != hipSuccess || lease.pinned(filterrows::kLitBlock + filterrows::kCtrlBytes, &pinned) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "filter rows: " + std::to_string(at.total) + " B of block counts and their scan");
    }
    uint8_t* b = (uint8_t*)base;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    const unsigned long long* h_ctrl = (const unsigned long long*)((uint8_t*)pinned + filterrows::kLitBlock);
    uint32_t* d_counts = d_idx ? (uint32_t*)(b + at.counts) : nullptr;
    uint64_t* d_bases = (uint64_t*)(b + at.bases);
    unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
    if (d_idx && !d_mask) d_mask = (uint64_t*)(b + at.mask);
    int rc = [&]() -> int {
        if (!lits.bytes.empty()) {
            memcpy(pinned, lits.bytes.data(), lits.bytes.size());
            HIP_TRY(hipMemcpyAsync(b + at.lits, pinned, lits.bytes.size(), hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kFilterCtrlWords * 8, st));
        filter_eval_kernel<<<eval_grid(n), 256, 0, st>>>(call, (const uint64_t*)(b + at.lits), n, d_mask, d_counts, d_ctrl);
        HIP_TRY(hipGetLastError());
        if (d_idx) {
            int r = exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st);
            if (r) return r;
            filter_emit_kernel<<<stride_grid(n), 256, 0, st>>>(d_mask, d_bases, n, d_idx, d_ctrl);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync((uint8_t*)pinned + filterrows::kLitBlock, d_ctrl, kFilterCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) {
        (void)hipStreamSynchronize(st);  // work of a failed call may still be queued
        return rc;
    }
    if (h_ctrl[kFilterCtrlErr] & kFilterErrPlace)
        return fail(OXH_ERR_HIP, "filter rows: a place is not among the selected rows at or before its row (the columns changed during the call?); no result");
    stats2[0] = h_ctrl[kFilterCtrlSelected], stats2[1] = h_ctrl[kFilterCtrlNull];
    STEP("filter rows: %llu rows, %u terms, %llu selected, %llu null", (unsigned long long)n, a.nterms, (unsigned long long)stats2[0],
         (unsigned long long)stats2[1]);
    if (h_ctrl[kFilterCtrlErr])  // the outputs are those of the frame with the bad cells empty
        return fail(OXH_ERR_INVALID, "filter rows: a byte column's offsets decrease or are negative, or it has bytes but no values");
    return OXH_OK;
}

// What both forms do before they need a device. `done`: no rows, nothing left to do.
int filter_enter(oxh_ctx* ctx, const filterrows::Args& a, bool host, bool& done) {
    done = false;
    const std::string what = filterrows::argument_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "filter rows: " + what);
    if (a.nrows == 0) {
        a.stats2[0] = a.stats2[1] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

}  // namespace

extern "C" {

int oxh_filter_rows_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                           const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                           const uint32_t* orders, uint32_t nterms, const uint32_t* term_col, const uint32_t* term_op,
                           const uint64_t* term_word, const uint8_t* lit_bytes, const uint64_t* lit_offsets,
                           const uint32_t* logical, uint32_t* d_idx, uint64_t* d_mask, uint64_t* stats2, void* stream) {
    const filterrows::Args a{nrows, ncols, kinds, d_values, d_offsets, d_validity, bit_offsets, orders, nterms, term_col,
                             term_op, term_word, lit_bytes, lit_offsets, logical, d_idx, d_mask, stats2};
    bool done = false;
    int rc = filter_enter(ctx, a, false, done);
    if (rc || done) return rc;
    return filter_rows_run(a, d_values, d_offsets, d_validity, bit_offsets, d_idx, d_mask, stats2, (hipStream_t)stream);
}

int oxh_filter_rows_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* kinds, const void* const* values,
                         const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                         const uint32_t* orders, uint32_t nterms, const uint32_t* term_col, const uint32_t* term_op,
                         const uint64_t* term_word, const uint8_t* lit_bytes, const uint64_t* lit_offsets,
                         const uint32_t* logical, uint32_t* idx, uint64_t* mask, uint64_t* stats2) {
    const filterrows::Args a{nrows, ncols, kinds, values, offsets, validity, bit_offsets, orders, nterms, term_col,
                             term_op, term_word, lit_bytes, lit_offsets, logical, idx, mask, stats2};
    bool done = false;
    int rc = filter_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // One device block: idx and the mask, then for every column a term names only what its rows name (columns.hpp).
    const filterrows::HostPlan plan(a);
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, plan.staging.total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "filter rows: " + std::to_string(plan.staging.total) + " B for the named columns on the device");
    }
    oxh::poison_device(d_block, plan.staging.total + 16, st);
    uint64_t stats[2] = {0, 0};
    std::vector<uint32_t> out_idx;
    std::vector<uint64_t> out_mask;
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : plan.staging.pieces)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(d_block + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        std::vector<const void*> d_values(ncols, nullptr), d_offsets(ncols, nullptr);
        std::vector<const uint8_t*> d_validity(ncols, nullptr);
        std::vector<uint64_t> bits(2 * (size_t)ncols, 0);
        for (uint32_t c = 0; c < ncols; ++c) {
            if (plan.staged_of[c] < 0) continue;  // no term names it
            const oxh::cols::Staged& s = plan.staged[plan.staged_of[c]];
            d_values[c] = plan.staging.values_at(d_block, s);
            d_offsets[c] = plan.staging.offsets_at(d_block, s);
            d_validity[c] = plan.staging.validity_at(d_block, s);
            bits[2 * c] = s.vbit, bits[2 * c + 1] = s.nbit;
        }
        uint32_t* d_idx = idx ? (uint32_t*)d_block : nullptr;
        uint64_t* d_mask = mask ? (uint64_t*)(d_block + plan.idx_bytes) : nullptr;
        int r = filter_rows_run(a, d_values.data(), d_offsets.data(), d_validity.data(), bits.data(), d_idx, d_mask, stats, st);
        if (r) return r;
        // the caller's arrays stay untouched unless everything succeeded
        if (idx && stats[0]) {
            out_idx.resize(stats[0]);
            HIP_TRY(hipMemcpyAsync(out_idx.data(), d_idx, stats[0] * 4, hipMemcpyDeviceToHost, st));
        }
        if (mask) {
            out_mask.resize(filterrows::blocks_of(nrows));
            HIP_TRY(hipMemcpyAsync(out_mask.data(), d_mask, out_mask.size() * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    if (rc) return rc;
    if (!out_idx.empty()) memcpy(idx, out_idx.data(), out_idx.size() * 4);
    if (!out_mask.empty()) memcpy(mask, out_mask.data(), out_mask.size() * 8);
    memcpy(stats2, stats, sizeof stats);
    return OXH_OK;
}

}  // extern "C"
