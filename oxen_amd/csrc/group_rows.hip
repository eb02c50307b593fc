// oxen_amd/csrc/group_rows.hip -- the rows of a frame grouped by equality on key columns (oxh_group_rows_*):
// `oxen df --unique` (core/df/tabular.rs:424-427 unique_df: df.unique(Some(columns), UniqueKeepStrategy::First)),
// `--unique_count` (:429-433 unique_count_df: group_by(cols).agg([len()])) and the count of duplicated rows
// (:263-271 n_duped_rows: select(cols).is_duplicated().sum()), from the key columns (Arrow: values, offsets,
// validity bitmaps) on the device. The equality is stated in include/oxen_hash.h (DESIGN.md §4 "Group").
//
// One call is, on one stream:
//   image    the digest of every row's KEY IMAGE (columns.hpp image_cell: a tag per cell, floats in
//            sort_keys.hpp's canonical word, byte cells behind their length): injective over rows and the same
//            for equal rows, which the row hashes' undelimited bytes are not. The kernels are row_hash.hip's,
//            instantiated for that image: a length pass, one lane per row of at most 240 encoded bytes with
//            the image in its LDS slot, the arena and the packed K1 for the longer ones;
//   index    the digests go into a private dedup index through its public entries: first[i] = the smallest
//            row that carries row i's digest = group[i];
//   count    group_count_kernel, one lane per row, grid-stride: count_of[group[i]] += 1 -- a run of equal
//            neighbours in a wave adds its length once (wave_runs), into the workgroup's table in LDS, which
//            goes to memory with one relaxed agent-scope atomic per id when the loop has ended; what finds no
//            place in the table adds straight to memory; group[i] and the flag group[i] == i;
//   scan     exclusive_scan_u32 over the flags: a first occurrence's place among the first occurrences;
//   emit     group_emit_kernel, a later launch, so every add has landed: count[i] = count_of[group[i]],
//            first_idx / first_count at the scanned place, and the four stats reduced per wave (ballots and
//            shuffles), per workgroup (LDS), then one atomic each.
// No lane ever waits for another lane or workgroup; launches order the steps. An id from the index that is
// not a row at or before its own is never used as an index: it sets the error word (OXH_ERR_HIP). A place
// from the scan is checked against the row before it is stored through.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "group_rows_host.hpp"

using namespace oxh::capi;

namespace oxh {

constexpr unsigned long long kGroupErrId = 1, kGroupErrPlace = 2;
// ctrl words of one call: the error word, then stats4[0..2]
constexpr int kGroupCtrlErr = 0, kGroupCtrlGroups = 1, kGroupCtrlDuplicated = 2, kGroupCtrlLargest = 3, kGroupCtrlWords = 4;

// The count's table in LDS: a workgroup sums the rows of an id there first and adds every sum once when its
// loop has ended, so a frame of few large groups (`--unique_count label`: millions of rows on a hundred ids)
// costs a few global atomics per workgroup and id, not one per row or run. Open addressing, kGroupProbes
// places per id; no new id is taken once three quarters are in use (a frame of distinct rows fills it at
// once and then pays a few LDS reads per row); whatever finds no place adds straight to memory.
constexpr uint32_t kGroupSlots = 512, kGroupProbes = 4, kGroupEmpty = 0xFFFFFFFFu;  // no row is 2^32 - 1

// count_of[g] = the rows whose id is g (zeroed before); group[i] (may be NULL) and flag[i] = id == i.
__global__ __launch_bounds__(256) void group_count_kernel(const uint64_t* __restrict__ first, uint64_t n, uint32_t* __restrict__ count_of,
                                                          uint32_t* __restrict__ flag, uint32_t* __restrict__ group,
                                                          unsigned long long* __restrict__ ctrl) {
    __shared__ uint32_t slot_id[kGroupSlots], slot_sum[kGroupSlots], used;
    for (uint32_t s = threadIdx.x; s < kGroupSlots; s += 256) slot_id[s] = kGroupEmpty, slot_sum[s] = 0;
    if (threadIdx.x == 0) used = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the shuffles and the barrier
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool live = i < n;
        const uint64_t g = live ? first[i] : 0;
        if (live && g > i) {  // not a row at or before this one: never index count_of with it
            __hip_atomic_fetch_or(&ctrl[kGroupCtrlErr], kGroupErrId, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            flag[i] = 0;
            if (group) group[i] = (uint32_t)i;
            live = false;
        }
        bool head;
        uint32_t len, rank;
        unsigned head_lane;
        wave_runs(live ? g : ~0ull, lane, head, len, rank, head_lane);
        if (!live) continue;
        flag[i] = g == i;
        if (group) group[i] = (uint32_t)g;
        if (!head) continue;
        bool placed = false;
        const uint32_t id = (uint32_t)g;
        uint32_t s = (id * 0x9E3779B1u) >> 23;  // 9 bits: kGroupSlots places
        for (uint32_t p = 0; p < kGroupProbes && !placed; ++p, s = (s + 1) & (kGroupSlots - 1)) {
            uint32_t k = __hip_atomic_load(&slot_id[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (k == kGroupEmpty) {
                if (__hip_atomic_load(&used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= kGroupSlots / 4 * 3) break;
                k = atomicCAS(&slot_id[s], kGroupEmpty, id);  // a place never changes once it is taken
                if (k == kGroupEmpty) {
                    atomicAdd(&used, 1u);
                    k = id;
                }
            }
            if (k == id) {
                atomicAdd(&slot_sum[s], len);
                placed = true;
            }
        }
        if (!placed) __hip_atomic_fetch_add(&count_of[g], len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kGroupSlots; s += 256) {
        const uint32_t id = slot_id[s];  // an id here was checked against its row above
        if (id != kGroupEmpty) __hip_atomic_fetch_add(&count_of[id], slot_sum[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// (every add of the count has landed, the flags are scanned) count[i]; first_idx / first_count at the place
// of every first occurrence; the stats. Any of the three outputs may be NULL.
__global__ __launch_bounds__(256) void group_emit_kernel(const uint64_t* __restrict__ first, uint64_t n,
                                                         const uint32_t* __restrict__ count_of, const uint64_t* __restrict__ place_of,
                                                         uint32_t* __restrict__ count, uint32_t* __restrict__ first_idx,
                                                         uint32_t* __restrict__ first_count, unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long part[4][3];
    unsigned long long groups = 0, duplicated = 0, bad = 0;
    uint32_t largest = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool is_first = false, is_dup = false;
        if (i < n) {
            const uint64_t g = first[i];
            if (g <= i) {  // else the count kernel has set the error word
                const uint32_t c = count_of[g];
                if (count) count[i] = c;
                is_first = g == i;
                is_dup = c >= 2;
                largest = c > largest ? c : largest;
                if (is_first) {
                    const uint64_t place = place_of[i];
                    if (place <= i) {  // the first occurrences before row i: never a store outside the n places
                        if (first_idx) first_idx[place] = (uint32_t)i;
                        if (first_count) first_count[place] = c;
                    } else {
                        bad |= kGroupErrPlace;
                    }
                }
            }
        }
        groups += __popcll(__ballot(is_first));
        duplicated += __popcll(__ballot(is_dup));
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kGroupCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every lane is here
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t m = (uint32_t)__shfl_xor((int)largest, off, 64);
        largest = m > largest ? m : largest;
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* mine = part[threadIdx.x >> 6];
        mine[0] = groups, mine[1] = duplicated, mine[2] = largest;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (sum) atomicAdd(&ctrl[kGroupCtrlGroups + threadIdx.x], sum);
    } else if (threadIdx.x == 2) {
        unsigned long long m = 0;
        for (int w = 0; w < 4; ++w) m = part[w][2] > m ? part[w][2] : m;
        if (m) atomicMax(&ctrl[kGroupCtrlLargest], m);
    }
}

}  // namespace oxh

namespace {

namespace grouprows = oxh::grouprows;

unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 2048); }

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// One call over device-resident key columns; the outputs that were asked for are filled and the stream has
// drained on return. Everything row-shaped is one lease (group_rows_host.hpp's Lease and the long rows'
// scratch behind it); the index is private and sized for the rows.
int group_rows_run(oxh_ctx* ctx, const grouprows::Args& a, const void* const* d_values, const void* const* d_offsets,
                   const uint8_t* const* d_validity, const uint64_t* bits, uint32_t* d_group, uint32_t* d_count,
                   uint32_t* d_first_idx, uint32_t* d_first_count, hipStream_t st) {
    using namespace oxh;
    const uint64_t n = a.nrows;
    RowImageCall images;  // its block is freed after the lease has ended (and waited for the stream)
    int rc = images.measure(true, n, a.nkeys, a.kinds, a.orders, d_values, d_offsets, d_validity, bits, st);
    if (rc) return rc;
    CallBlock ctrl;
    if ((rc = ctrl.make(kGroupCtrlWords * 8, "group rows", st))) return rc;
    unsigned long long* d_ctrl = (unsigned long long*)ctrl.d;
    const unsigned long long* h_ctrl = (const unsigned long long*)ctrl.h;
    void* index = nullptr;
    if ((rc = oxh_dedup_index_create(ctx, n, &index))) return rc;
    rc = [&]() -> int {
        const grouprows::Lease at(n);
        if (grouprows::scan_tiles_of(n) != scan_tiles(n)) return fail(OXH_ERR_HIP, "group rows: the scan's tile is not the lease's");
        ScratchLease lease(st);  // ends (and waits for the stream) before the index and the blocks are freed
        void* base = nullptr;
        const uint64_t total = at.total + images.scratch_bytes();
        if (lease.get(total, &base) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "group rows: " + std::to_string(total) + " B of digests, ids and counts");
        }
        uint8_t* b = (uint8_t*)base;
        uint64_t* d_digests = (uint64_t*)(b + at.digests);
        uint64_t* d_first = (uint64_t*)(b + at.first);
        uint32_t* d_count_of = (uint32_t*)(b + at.count_of);
        uint32_t* d_flag = (uint32_t*)(b + at.flag);
        uint64_t* d_place = (uint64_t*)(b + at.flag_scan);
        unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
        int r = images.hash(d_digests, b + at.total, st);
        if (r) return r;
        if ((r = oxh_dedup_index_insert_device(index, d_digests, nullptr, n, d_first, nullptr, st))) return r;
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kGroupCtrlWords * 8, st));
        HIP_TRY(hipMemsetAsync(d_count_of, 0, n * 4, st));
        group_count_kernel<<<stride_grid(n), 256, 0, st>>>(d_first, n, d_count_of, d_flag, d_group, d_ctrl);
        HIP_TRY(hipGetLastError());
        if ((r = exclusive_scan_u32(d_flag, n, d_place, d_sums, st))) return r;
        group_emit_kernel<<<stride_grid(n), 256, 0, st>>>(d_first, n, d_count_of, d_place, d_count, d_first_idx, d_first_count, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ctrl.h, d_ctrl, kGroupCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_ctrl[kGroupCtrlErr])
            return fail(OXH_ERR_HIP, "group rows: an id or a place is not a row at or before its own (the keys changed during the call?); no result");
        a.stats4[0] = h_ctrl[kGroupCtrlGroups], a.stats4[1] = h_ctrl[kGroupCtrlDuplicated];
        a.stats4[2] = h_ctrl[kGroupCtrlLargest], a.stats4[3] = images.nlong;
        STEP("group rows: %llu rows in %llu groups, %llu duplicated, the largest %llu, %llu long", (unsigned long long)n,
             (unsigned long long)a.stats4[0], (unsigned long long)a.stats4[1], (unsigned long long)a.stats4[2],
             (unsigned long long)a.stats4[3]);
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);  // work of a failed call may still be queued
    (void)oxh_dedup_index_destroy(index);
    if (rc) return rc;
    if (images.deferred == OXH_ERR_INVALID)  // the outputs are those of the frame with the bad cells empty
        return fail(OXH_ERR_INVALID, "group rows: a byte column's offsets decrease or are negative, or it has bytes but no values");
    return images.deferred;
}

// What both forms do before they need a device. `done`: no rows, nothing left to do.
int group_enter(oxh_ctx* ctx, const grouprows::Args& a, bool host, bool& done) {
    done = false;
    const std::string what = grouprows::argument_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "group rows: " + what);
    if (a.nrows == 0) {
        a.stats4[0] = a.stats4[1] = a.stats4[2] = a.stats4[3] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

}  // namespace

extern "C" {

int oxh_group_rows_device(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* d_values,
                          const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                          const uint32_t* orders, uint32_t* d_group, uint32_t* d_count, uint32_t* d_first_idx,
                          uint32_t* d_first_count, uint64_t* stats4, void* stream) {
    const grouprows::Args a{nrows, nkeys, kinds, d_values, d_offsets, d_validity, bit_offsets, orders,
                            d_group, d_count, d_first_idx, d_first_count, stats4};
    bool done = false;
    int rc = group_enter(ctx, a, false, done);
    if (rc || done) return rc;
    return group_rows_run(ctx, a, d_values, d_offsets, d_validity, bit_offsets, d_group, d_count, d_first_idx, d_first_count,
                          (hipStream_t)stream);
}

int oxh_group_rows_host(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* values,
                        const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                        const uint32_t* orders, uint32_t* group, uint32_t* count, uint32_t* first_idx, uint32_t* first_count,
                        uint64_t* stats4) {
    const grouprows::Args a{nrows, nkeys, kinds, values, offsets, validity, bit_offsets, orders, group, count, first_idx, first_count, stats4};
    bool done = false;
    int rc = group_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // One device block: the four output arrays, then for every key column only what its rows name (columns.hpp).
    const grouprows::HostPlan plan(a);
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, plan.staging.total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "group rows: " + std::to_string(plan.staging.total) + " B for the key columns on the device");
    }
    oxh::poison_device(d_block, plan.staging.total + 16, st);
    uint64_t stats[4] = {0, 0, 0, 0};
    uint32_t* const wanted[4] = {group, count, first_idx, first_count};
    std::vector<uint32_t> out[4];
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : plan.staging.pieces)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(d_block + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        std::vector<const void*> d_values(nkeys), d_offsets(nkeys);
        std::vector<const uint8_t*> d_validity(nkeys);
        std::vector<uint64_t> bits(2 * (size_t)nkeys, 0);
        for (uint32_t c = 0; c < nkeys; ++c) {
            d_values[c] = plan.staging.values_at(d_block, plan.staged[c]);
            d_offsets[c] = plan.staging.offsets_at(d_block, plan.staged[c]);
            d_validity[c] = plan.staging.validity_at(d_block, plan.staged[c]);
            bits[2 * c] = plan.staged[c].vbit, bits[2 * c + 1] = plan.staged[c].nbit;
        }
        uint32_t* d_out[4];
        for (int k = 0; k < 4; ++k) d_out[k] = wanted[k] ? (uint32_t*)(d_block + k * plan.out_bytes) : nullptr;
        grouprows::Args d = a;
        d.stats4 = stats;
        int r = group_rows_run(ctx, d, d_values.data(), d_offsets.data(), d_validity.data(), bits.data(), d_out[0], d_out[1], d_out[2],
                               d_out[3], st);
        if (r) return r;
        // the caller's arrays stay untouched unless everything succeeded
        for (int k = 0; k < 4; ++k) {
            if (!wanted[k]) continue;
            const uint64_t rows = k < 2 ? nrows : stats[0];
            out[k].resize(rows);
            if (rows) HIP_TRY(hipMemcpyAsync(out[k].data(), d_out[k], rows * 4, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    if (rc) return rc;
    for (int k = 0; k < 4; ++k)
        if (wanted[k] && !out[k].empty()) memcpy(wanted[k], out[k].data(), out[k].size() * 4);
    memcpy(stats4, stats, sizeof stats);
    return OXH_OK;
}

}  // extern "C"
