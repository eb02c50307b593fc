// oxen_amd/csrc/keyed_diff.hip -- the keyed tabular diff (oxh_keyed_diff_*): `oxen diff --keys ... --targets
// ...` after the row hashes. The reference full-joins the two hashed frames on the key hash
// (repositories/diffs/join_diff.rs:290), walks the joined frame row by row through `test_function`
// (:458-484), filters the unchanged rows out (:88-92), counts the rest (:434-456) and counts the rows of
// duplicated keys (core/df/tabular.rs:263-271). Here the four digest tables stay on the device and one call
// returns the classified row pairs and the summary (DESIGN.md §4 "Keyed diff").
//
// Rows [0, nl) are left, [nl, n) right: a row's ordinal. One insert of the left then the right key digests
// into a private dedup index (oxh_dedup_index_*, through its public entries) gives every row its id, the
// smallest ordinal that carries its key. A group -- the rows of one key -- has four words at grp[4 * id]:
//   [0] left rows, [1] right rows, [2] 1 + some right row of it (the partner, when there is one right row)
//   or, in a group with a bucket, the fill cursor; [3] where its bucket starts.
// A group with a left row and two or more right rows has a bucket: its right rows, contiguous in `bucket`.
// One call is, on one stream:
//   count     grp[0] / grp[1] += 1 per row (a run of equal neighbours in a wave adds once), grp[2];
//   plan      the row whose ordinal is its id gives its group a bucket: an exclusive prefix sum of the
//             sizes inside the workgroup on top of what one atomic add per workgroup returns;
//   bucket    every right row of such a group takes the next place of its bucket (atomic cursor);
//   classify  one lane per row walks the row's joined rows -- a left row its partners or (l, none), a right
//             row (none, r) when its group has no left row -- and counts them by status, the rows of
//             duplicated keys, and emit[row] = how many of them the call emits;
//   scan      off[] = the exclusive prefix sum of emit[] (exclusive_scan_u32: three launches);
//   fill      (only when the pairs fit the caller's capacity) the same walk writes the pairs at off[row].
// No lane ever waits for another lane or workgroup. Every id, partner, bucket place and output place read
// from device memory is checked before it is used; a bad one sets the error word (OXH_ERR_HIP).
#include "capi_internal.hpp"
#include "keyed_diff_host.hpp"

using namespace oxh::capi;

namespace oxh {

// ---------------------------------------------------------------- device-wide exclusive scan
// off[i] = in[0] + ... + in[i-1] over n u32, as u64; sums[ntiles] = the total. Three launches: the sum of
// every tile of kScanTile elements, one workgroup that scans those sums, and the scan inside every tile on
// top of its tile's sum. No workgroup waits for another (no look-back): the launches order the steps.
constexpr uint32_t kScanPer = 8, kScanTile = 256 * kScanPer;

// The exclusive prefix sum of v over the 256 lanes of the workgroup; total = their sum. Every lane calls it
// (two barriers); wave_sum is 4 words of LDS, free again at the next call's first barrier.
__device__ __forceinline__ unsigned long long block_scan256(unsigned long long v, unsigned long long* wave_sum,
                                                            unsigned long long& total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, off, 64);
        if (lane >= (unsigned)off) incl += up;
    }
    __syncthreads();  // the words of an earlier call have been read
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned long long base = 0;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        base += w < wave ? wave_sum[w] : 0;
        total += wave_sum[w];
    }
    return base + incl - v;
}

__global__ __launch_bounds__(256) void scan_tile_sums_kernel(const uint32_t* __restrict__ in, uint64_t n, uint64_t ntiles,
                                                             unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long wave_sum[4];
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform over the workgroup
        const uint64_t at = tile * kScanTile + (uint64_t)threadIdx.x * kScanPer;
        unsigned long long mine = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; ++k) mine += at + k < n ? in[at + k] : 0;
        (void)block_scan256(mine, wave_sum, total);
        if (threadIdx.x == 0) sums[tile] = total;
    }
}

// One workgroup: sums[0 .. ntiles) to their exclusive prefix sums, in place; sums[ntiles] = the total.
__global__ __launch_bounds__(256) void scan_sums_kernel(unsigned long long* __restrict__ sums, uint64_t ntiles) {
    __shared__ unsigned long long wave_sum[4];
    unsigned long long carry = 0;  // the same in every lane
    for (uint64_t base = 0; base < ntiles; base += 256) {
        const uint64_t t = base + threadIdx.x;
        const unsigned long long v = t < ntiles ? sums[t] : 0;
        unsigned long long total = 0;
        const unsigned long long before = block_scan256(v, wave_sum, total);
        if (t < ntiles) sums[t] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) sums[ntiles] = carry;
}

__global__ __launch_bounds__(256) void scan_apply_kernel(const uint32_t* __restrict__ in, uint64_t n, uint64_t ntiles,
                                                         const unsigned long long* __restrict__ sums,
                                                         uint64_t* __restrict__ out) {
    __shared__ unsigned long long wave_sum[4];
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t at = tile * kScanTile + (uint64_t)threadIdx.x * kScanPer;
        uint32_t v[kScanPer];
        unsigned long long mine = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; ++k) {
            v[k] = at + k < n ? in[at + k] : 0;
            mine += v[k];
        }
        unsigned long long run = sums[tile] + block_scan256(mine, wave_sum, total);
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; ++k) {
            if (at + k < n) out[at + k] = run;
            run += v[k];
        }
    }
}

uint64_t scan_tiles(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }

int exclusive_scan_u32(const uint32_t* d_in, uint64_t n, uint64_t* d_out, unsigned long long* d_sums, hipStream_t st) {
    const uint64_t ntiles = scan_tiles(n);
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>(ntiles, 1), 2048);
    scan_tile_sums_kernel<<<grid, 256, 0, st>>>(d_in, n, ntiles, d_sums);
    HIP_TRY(hipGetLastError());
    scan_sums_kernel<<<1, 256, 0, st>>>(d_sums, ntiles);
    HIP_TRY(hipGetLastError());
    scan_apply_kernel<<<grid, 256, 0, st>>>(d_in, n, ntiles, d_sums, d_out);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

// ---------------------------------------------------------------- keyed diff
constexpr unsigned long long kKeyedErrId = 1, kKeyedErrPartner = 2, kKeyedErrBucket = 4, kKeyedErrPlace = 8;
// ctrl words of one call: the error word, the joined rows by status (at kCtrlStatus + OXH_DIFF_*), the rows
// of duplicated keys left / right, the bucket cursor
constexpr int kCtrlErr = 0, kCtrlStatus = 1, kCtrlDupes = 5, kCtrlCursor = 7, kCtrlWords = 8;
constexpr uint32_t kNone = OXH_KEYED_DIFF_NONE;

struct KeyedArgs {
    const uint64_t* id;                    // n: each row's id
    uint32_t* grp;                         // 4 n, 16-B aligned
    uint32_t* emit;                        // n
    uint64_t* off;                         // n
    uint32_t* bucket;                      // nr, 0xFF-filled: an unfilled place is no row
    const uint64_t *ltarget, *rtarget;     // NULL: the null column
    const uint8_t *lvalid, *rvalid;        // NULL: no nulls
    uint64_t lbit, rbit;
    uint64_t nl, n;
    uint32_t *left_idx, *right_idx;        // fill: `total` places each
    uint8_t* status;
    uint64_t total;
    unsigned long long* ctrl;
    uint32_t keep;
};

__device__ __forceinline__ bool keyed_bit(const uint8_t* p, uint64_t bit) { return !p || ((p[bit >> 3] >> (bit & 7)) & 1); }

// grp[0] / grp[1] of every group, and grp[2] = 1 + a right row of it. The adds of a run of equal
// neighbours (a region of one key) are one add of the run's length, as the index's insert spares its probes.
__global__ __launch_bounds__(256) void keyed_count_kernel(KeyedArgs a) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (a.n + stride - 1) / stride;  // uniform: every lane reaches the shuffles
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool live = i < a.n;
        const uint64_t g = live ? a.id[i] : 0;
        if (live && g >= a.n) {  // not an ordinal of this call: never index grp with it
            __hip_atomic_fetch_or(&a.ctrl[kCtrlErr], kKeyedErrId, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            live = false;
        }
        const unsigned side = i >= a.nl;
        bool head;
        uint32_t len, rank;
        unsigned head_lane;
        wave_runs(live ? 2 * g + side : ~0ull, lane, head, len, rank, head_lane);
        if (!live || !head) continue;
        __hip_atomic_fetch_add(&a.grp[4 * g + side], len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // any right row of the group: it is read only where the group has exactly one
        if (side) __hip_atomic_store(&a.grp[4 * g + 2], (uint32_t)(i - a.nl) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ bool keyed_has_bucket(uint32_t nleft, uint32_t nright) { return nleft >= 1 && nright >= 2; }

// (every add of the count has landed) The row whose ordinal is its id stands for its group: where the
// group has a bucket, grp[3] = its start and grp[2] = 0, the fill cursor. Which workgroup's buckets come
// first is not fixed; only the order inside a bucket can show, and only in the device form.
__global__ __launch_bounds__(256) void keyed_plan_kernel(KeyedArgs a) {
    __shared__ unsigned long long wave_sum[4], wg_base;
    const uint64_t nbucket = a.n - a.nl;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (a.n + stride - 1) / stride;  // uniform: every lane reaches the barriers
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t g = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        unsigned long long need = 0, total = 0;
        if (g < a.n && a.id[g] == g && keyed_has_bucket(a.grp[4 * g], a.grp[4 * g + 1])) need = a.grp[4 * g + 1];
        const unsigned long long before = block_scan256(need, wave_sum, total);
        if (threadIdx.x == 0) wg_base = total ? atomicAdd(&a.ctrl[kCtrlCursor], total) : 0;
        __syncthreads();
        if (!need) continue;
        const unsigned long long start = wg_base + before;
        if (start > nbucket || need > nbucket - start) {  // more than the right rows there are
            __hip_atomic_fetch_or(&a.ctrl[kCtrlErr], kKeyedErrBucket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        a.grp[4 * g + 2] = 0;
        a.grp[4 * g + 3] = (uint32_t)start;
    }
}

// Every right row of a group with a bucket takes the next place in it; a run of equal neighbours takes its
// places with one add.
__global__ __launch_bounds__(256) void keyed_bucket_kernel(KeyedArgs a) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t nr = a.n - a.nl;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (nr + stride - 1) / stride;  // uniform: every lane reaches the shuffles
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t j = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool live = j < nr;
        const uint64_t g = live ? a.id[a.nl + j] : 0;
        if (live && g >= a.n) live = false;  // the count has set the error word
        uint32_t size = 0, start = 0;
        if (live) {
            size = a.grp[4 * g + 1];
            start = a.grp[4 * g + 3];
            live = keyed_has_bucket(a.grp[4 * g], size);
        }
        bool head;
        uint32_t len, rank;
        unsigned head_lane;
        wave_runs(live ? g : ~0ull, lane, head, len, rank, head_lane);
        uint32_t first = 0;
        if (live && head) first = __hip_atomic_fetch_add(&a.grp[4 * g + 2], len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        first = (uint32_t)__shfl((int)first, (int)head_lane, 64);
        if (!live) continue;
        const uint64_t place = (uint64_t)first + rank;
        if (place >= size || start + place >= nr) {  // more rows than the count saw
            __hip_atomic_fetch_or(&a.ctrl[kCtrlErr], kKeyedErrBucket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        a.bucket[start + place] = (uint32_t)j;
    }
}

// The status of the joined row (l, r), both present: test_function's order (join_diff.rs:458-484).
__device__ __forceinline__ uint32_t keyed_pair_status(const KeyedArgs& a, bool lvalid, uint64_t l, uint64_t r) {
    if (!lvalid) return OXH_DIFF_ADDED;
    if (!keyed_bit(a.rvalid, a.rbit + r)) return OXH_DIFF_REMOVED;
    if (!a.ltarget && !a.rtarget) return OXH_DIFF_UNCHANGED;
    if (!a.ltarget || !a.rtarget) return OXH_DIFF_MODIFIED;  // a null column against a digest
    return a.ltarget[2 * l] != a.rtarget[2 * r] || a.ltarget[2 * l + 1] != a.rtarget[2 * r + 1] ? OXH_DIFF_MODIFIED
                                                                                                 : OXH_DIFF_UNCHANGED;
}

// Row i's joined rows, in the order the call emits them. FILL: written from off[i] on; else counted into
// c[status] and c[4] / c[5] (a row of a duplicated key, left / right), and emit[i] set.
template <bool FILL>
__device__ __forceinline__ void keyed_row(const KeyedArgs& a, uint64_t i, unsigned long long (&c)[6], unsigned long long& bad) {
    const uint64_t nr = a.n - a.nl, g = a.id[i];
    uint32_t emitted = 0;
    uint64_t at = FILL ? a.off[i] : 0;
    auto put = [&](uint32_t l, uint32_t r, uint32_t s) {
        const bool out = s != OXH_DIFF_UNCHANGED || a.keep;
        if constexpr (FILL) {
            if (!out) return;
            if (at >= a.total) {  // never past what the host made room for
                bad |= kKeyedErrPlace;
                return;
            }
            a.left_idx[at] = l;
            a.right_idx[at] = r;
            a.status[at] = (uint8_t)s;
            ++at;
        } else {
            c[s] += 1;
            emitted += out;
        }
    };
    if (g >= a.n) {
        bad |= kKeyedErrId;
    } else {
        const uint4 group = *reinterpret_cast<const uint4*>(a.grp + 4 * g);
        if (i < a.nl) {
            const bool lvalid = keyed_bit(a.lvalid, a.lbit + i);
            if (group.y == 0) {
                put((uint32_t)i, kNone, lvalid ? OXH_DIFF_REMOVED : OXH_DIFF_ADDED);
            } else if (group.y == 1) {
                const uint32_t r = group.z - 1;
                if (r >= nr) bad |= kKeyedErrPartner;
                else put((uint32_t)i, r, keyed_pair_status(a, lvalid, i, r));
            } else if (group.w > nr || group.y > nr - group.w) {
                bad |= kKeyedErrBucket;
            } else {
                for (uint32_t k = 0; k < group.y; ++k) {
                    const uint32_t r = a.bucket[group.w + k];
                    if (r >= nr) bad |= kKeyedErrPartner;
                    else put((uint32_t)i, r, keyed_pair_status(a, lvalid, i, r));
                }
            }
            if (!FILL && group.x > 1) c[4] += 1;
        } else {
            if (group.x == 0) put(kNone, (uint32_t)(i - a.nl), OXH_DIFF_ADDED);
            if (!FILL && group.y > 1) c[5] += 1;
        }
    }
    if constexpr (!FILL) a.emit[i] = emitted;
}

// (every bucket is filled) emit[] and the call's six counters: summed per lane over its rows, per wave by
// shuffles, the workgroup's four waves through LDS, then one atomic add per counter and workgroup.
__global__ __launch_bounds__(256) void keyed_classify_kernel(KeyedArgs a) {
    __shared__ unsigned long long part[4][6];
    unsigned long long c[6] = {0, 0, 0, 0, 0, 0}, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) keyed_row<false>(a, i, c, bad);
    if (bad) __hip_atomic_fetch_or(&a.ctrl[kCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every lane is here (nothing above returns)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) c[k] += (unsigned long long)__shfl_xor((long long)c[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; ++k) part[threadIdx.x >> 6][k] = c[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        // c[0..3] are the statuses in the order of OXH_DIFF_*, c[4..5] the dupes
        if (sum) atomicAdd(&a.ctrl[threadIdx.x < 4 ? kCtrlStatus + threadIdx.x : kCtrlDupes + threadIdx.x - 4], sum);
    }
}

// (off[] is scanned) every row writes its pairs at its offset
__global__ __launch_bounds__(256) void keyed_fill_kernel(KeyedArgs a) {
    unsigned long long c[6] = {0, 0, 0, 0, 0, 0}, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) keyed_row<true>(a, i, c, bad);
    if (bad) __hip_atomic_fetch_or(&a.ctrl[kCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oxh

namespace {

unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 2048); }
uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

int keyed_error(unsigned long long e) {
    if (!e) return OXH_OK;
    std::string m = "keyed diff: ";
    if (e & oxh::kKeyedErrId) m += "a row's id is not below the row count; ";
    if (e & oxh::kKeyedErrPartner) m += "a partner is no right row; ";
    if (e & oxh::kKeyedErrBucket) m += "a bucket does not lie inside the right rows; ";
    if (e & oxh::kKeyedErrPlace) m += "a pair's place is not below the number of pairs; ";
    return fail(OXH_ERR_HIP, m + "no result");
}

// One call's temporaries, all made before any work starts: a private index sized for the rows (its two
// inserts neither grow nor allocate) and one device block
//   [id n u64 | off n u64 | scan sums tiles+1 u64 | ctrl 8 u64 | grp 4n u32 | emit n u32 | bucket nr u32]
// with 8 pinned words for ctrl. Freed once the stream has drained.
struct KeyedCall {
    void* index = nullptr;
    uint8_t* d_block = nullptr;
    unsigned long long *d_sums = nullptr, *d_ctrl = nullptr, *h_ctrl = nullptr;
    uint64_t* d_id = nullptr;
    uint64_t nl = 0, nr = 0, n = 0, grp_bytes = 0, bucket_bytes = 0;
    oxh::KeyedArgs a{};

    int make(oxh_ctx* ctx, uint64_t nleft, uint64_t nright, hipStream_t st) {
        nl = nleft, nr = nright, n = nleft + nright;
        int rc = oxh_dedup_index_create(ctx, n, &index);
        if (rc) return rc;
        const uint64_t tiles = oxh::scan_tiles(n);
        const uint64_t sums_at = 2 * n * 8, ctrl_at = sums_at + (tiles + 1) * 8, grp_at = align16(ctrl_at + oxh::kCtrlWords * 8);
        grp_bytes = 4 * n * 4;
        bucket_bytes = nr * 4;
        const uint64_t emit_at = grp_at + grp_bytes, bucket_at = emit_at + n * 4;
        if (hipMalloc(&d_block, bucket_at + bucket_bytes + 16) != hipSuccess ||
            hipHostMalloc(&h_ctrl, oxh::kCtrlWords * 8, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "keyed diff: " + std::to_string(n) + " rows of ids, groups, offsets and buckets");
        }
        oxh::poison_device(d_block, bucket_at + bucket_bytes + 16, st), oxh::poison_pinned(h_ctrl, oxh::kCtrlWords * 8);
        d_id = (uint64_t*)d_block;
        d_sums = (unsigned long long*)(d_block + sums_at);
        d_ctrl = (unsigned long long*)(d_block + ctrl_at);
        a.id = d_id;
        a.off = d_id + n;
        a.grp = (uint32_t*)(d_block + grp_at);
        a.emit = (uint32_t*)(d_block + emit_at);
        a.bucket = (uint32_t*)(d_block + bucket_at);
        a.nl = nl, a.n = n;
        a.ctrl = d_ctrl;
        return OXH_OK;
    }

    // insert .. classify over device tables; counts8[0..6] known on return (complete)
    int classify(const uint64_t* d_lk, const uint64_t* d_rk, const uint64_t* d_lt, const uint64_t* d_rt, const uint8_t* d_lv,
                 const uint8_t* d_rv, uint64_t lbit, uint64_t rbit, uint32_t flags, uint64_t* counts8, hipStream_t st) {
        a.ltarget = d_lt, a.rtarget = d_rt;
        a.lvalid = d_lv, a.rvalid = d_rv, a.lbit = lbit, a.rbit = rbit;
        a.keep = flags & OXH_KEYED_DIFF_KEEP_UNCHANGED;
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, oxh::kCtrlWords * 8, st));
        HIP_TRY(hipMemsetAsync(a.grp, 0, grp_bytes, st));
        if (nr) HIP_TRY(hipMemsetAsync(a.bucket, 0xFF, bucket_bytes, st));
        int rc = OXH_OK;
        if (nl && (rc = oxh_dedup_index_insert_device(index, d_lk, nullptr, nl, d_id, nullptr, st))) return rc;
        if (nr && (rc = oxh_dedup_index_insert_device(index, d_rk, nullptr, nr, d_id + nl, nullptr, st))) return rc;
        oxh::keyed_count_kernel<<<stride_grid(n), 256, 0, st>>>(a);
        HIP_TRY(hipGetLastError());
        if (nl && nr) {  // a bucket needs rows on both sides
            oxh::keyed_plan_kernel<<<stride_grid(n), 256, 0, st>>>(a);
            HIP_TRY(hipGetLastError());
            oxh::keyed_bucket_kernel<<<stride_grid(nr), 256, 0, st>>>(a);
            HIP_TRY(hipGetLastError());
        }
        oxh::keyed_classify_kernel<<<stride_grid(n), 256, 0, st>>>(a);
        HIP_TRY(hipGetLastError());
        if ((rc = read_ctrl(st))) return rc;
        const unsigned long long* by_status = h_ctrl + oxh::kCtrlStatus;
        counts8[1] = by_status[OXH_DIFF_ADDED], counts8[2] = by_status[OXH_DIFF_REMOVED];
        counts8[3] = by_status[OXH_DIFF_MODIFIED], counts8[4] = by_status[OXH_DIFF_UNCHANGED];
        counts8[5] = h_ctrl[oxh::kCtrlDupes], counts8[6] = h_ctrl[oxh::kCtrlDupes + 1];
        counts8[0] = counts8[1] + counts8[2] + counts8[3] + (a.keep ? counts8[4] : 0);
        counts8[7] = 0;
        return OXH_OK;
    }

    // scan and fill: `total` = counts8[0] pairs to the three device arrays; complete on return
    int fill(uint64_t total, uint32_t* d_left, uint32_t* d_right, uint8_t* d_status, hipStream_t st) {
        a.left_idx = d_left, a.right_idx = d_right, a.status = d_status, a.total = total;
        int rc = oxh::exclusive_scan_u32(a.emit, n, a.off, d_sums, st);
        if (rc) return rc;
        oxh::keyed_fill_kernel<<<stride_grid(n), 256, 0, st>>>(a);
        HIP_TRY(hipGetLastError());
        return read_ctrl(st);
    }

    int read_ctrl(hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, oxh::kCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return keyed_error(h_ctrl[oxh::kCtrlErr]);
    }

    void release(hipStream_t st, bool failed) {
        if (failed && index) (void)hipStreamSynchronize(st);  // work of a failed call may still be queued
        if (d_block) (void)hipFree(d_block);
        if (h_ctrl) (void)hipHostFree(h_ctrl);
        if (index) (void)oxh_dedup_index_destroy(index);
    }
};

// What both forms do before they need a device. `done`: no rows at all, counts8 zeroed.
int keyed_enter(oxh_ctx* ctx, const uint64_t* lk, uint64_t nl, const uint64_t* rk, uint64_t nr, const uint64_t* lt,
                const uint64_t* rt, const uint64_t* bit_offsets2, uint32_t flags, uint64_t capacity, const uint32_t* left_idx,
                const uint32_t* right_idx, const uint8_t* status, uint64_t* counts8, bool& done) {
    done = false;
    if (const char* what = oxh::keyed::argument_error(lk, nl, rk, nr, lt, rt, bit_offsets2, flags, capacity, left_idx, right_idx,
                                                      status, counts8))
        return fail(OXH_ERR_INVALID, std::string("keyed diff: ") + what);
    if (nl + nr == 0) {
        memset(counts8, 0, 8 * sizeof(uint64_t));
        done = true;
        return OXH_OK;
    }
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

}  // namespace

extern "C" {

int oxh_keyed_diff_device(oxh_ctx* ctx, const uint64_t* d_left_keys, uint64_t nleft, const uint64_t* d_right_keys,
                          uint64_t nright, const uint64_t* d_left_targets, const uint64_t* d_right_targets,
                          const uint8_t* d_left_key0_valid, const uint8_t* d_right_key0_valid, const uint64_t* bit_offsets2,
                          uint32_t flags, uint64_t capacity, uint32_t* d_left_idx, uint32_t* d_right_idx, uint8_t* d_status,
                          uint64_t* counts8, void* stream) {
    bool done = false;
    int rc = keyed_enter(ctx, d_left_keys, nleft, d_right_keys, nright, d_left_targets, d_right_targets, bit_offsets2, flags,
                         capacity, d_left_idx, d_right_idx, d_status, counts8, done);
    if (rc || done) return rc;
    hipStream_t st = (hipStream_t)stream;
    KeyedCall call;
    uint64_t counts[8] = {};
    rc = call.make(ctx, nleft, nright, st);
    if (rc == OXH_OK)
        rc = call.classify(d_left_keys, d_right_keys, d_left_targets, d_right_targets, d_left_key0_valid, d_right_key0_valid,
                           bit_offsets2[0], bit_offsets2[1], flags, counts, st);
    if (rc == OXH_OK && counts[0] && counts[0] <= capacity) {
        rc = call.fill(counts[0], d_left_idx, d_right_idx, d_status, st);
        counts[7] = counts[0];
    }
    call.release(st, rc != OXH_OK);
    if (rc == OXH_OK) memcpy(counts8, counts, sizeof counts);
    return rc;
}

int oxh_keyed_diff_host(oxh_ctx* ctx, const uint64_t* left_keys, uint64_t nleft, const uint64_t* right_keys, uint64_t nright,
                        const uint64_t* left_targets, const uint64_t* right_targets, const uint8_t* left_key0_valid,
                        const uint8_t* right_key0_valid, const uint64_t* bit_offsets2, uint32_t flags, uint64_t capacity,
                        uint32_t* left_idx, uint32_t* right_idx, uint8_t* status, uint64_t* counts8) {
    bool done = false;
    int rc = keyed_enter(ctx, left_keys, nleft, right_keys, nright, left_targets, right_targets, bit_offsets2, flags, capacity,
                         left_idx, right_idx, status, counts8, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // One device block for the inputs: the tables that are there, then only the bytes that hold each
    // bitmap's bits (its residual bit offset is what the kernels get), each piece 16-B aligned. The pairs
    // get a block of their own once their number is known.
    struct Piece {
        const void* src;
        uint64_t bytes, at;
    };
    Piece pieces[6];
    int npieces = 0;
    uint64_t total = 0;
    auto add = [&](const void* src, uint64_t bytes) -> int {
        if (!src || !bytes) return -1;
        pieces[npieces] = {src, bytes, total};
        total += align16(bytes);
        return npieces++;
    };
    const int lk = add(left_keys, nleft * 16), rk = add(right_keys, nright * 16);
    const int lt = add(left_targets, nleft * 16), rt = add(right_targets, nright * 16);
    const uint64_t lbit = bit_offsets2[0] & 7, rbit = bit_offsets2[1] & 7;
    const int lv = left_key0_valid && nleft ? add(left_key0_valid + (bit_offsets2[0] >> 3), (lbit + nleft + 7) >> 3) : -1;
    const int rv = right_key0_valid && nright ? add(right_key0_valid + (bit_offsets2[1] >> 3), (rbit + nright + 7) >> 3) : -1;
    KeyedCall call;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint64_t counts[8] = {};
    rc = call.make(ctx, nleft, nright, st);
    if (rc == OXH_OK && hipMalloc(&d_in, total + 16) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(OXH_ERR_NOMEM, "keyed diff: " + std::to_string(total) + " B for the tables on the device");
    }
    oxh::poison_device(d_in, total + 16, st);
    if (rc == OXH_OK)
        rc = [&]() -> int {
            for (int k = 0; k < npieces; ++k)
                HIP_TRY(hipMemcpyAsync(d_in + pieces[k].at, pieces[k].src, pieces[k].bytes, hipMemcpyHostToDevice, st));
            auto at = [&](int piece) { return piece < 0 ? nullptr : d_in + pieces[piece].at; };
            int r = call.classify((const uint64_t*)at(lk), (const uint64_t*)at(rk), (const uint64_t*)at(lt), (const uint64_t*)at(rt),
                                  at(lv), at(rv), lbit, rbit, flags, counts, st);
            if (r || !counts[0] || counts[0] > capacity) return r;
            const uint64_t pairs = counts[0], right_at = align16(pairs * 4), status_at = 2 * right_at;
            if (hipMalloc(&d_out, status_at + pairs) != hipSuccess) {
                (void)hipGetLastError();
                return fail(OXH_ERR_NOMEM, "keyed diff: " + std::to_string(pairs) + " pairs on the device");
            }
            oxh::poison_device(d_out, status_at + pairs, st);
            if ((r = call.fill(pairs, (uint32_t*)d_out, (uint32_t*)(d_out + right_at), d_out + status_at, st))) return r;
            HIP_TRY(hipMemcpyAsync(left_idx, d_out, pairs * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(right_idx, d_out + right_at, pairs * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(status, d_out + status_at, pairs, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            oxh::keyed::sort_runs(left_idx, right_idx, status, pairs);
            counts[7] = pairs;
            return OXH_OK;
        }();
    call.release(st, rc != OXH_OK);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (rc == OXH_OK) memcpy(counts8, counts, sizeof counts);
    return rc;
}

}  // extern "C"
