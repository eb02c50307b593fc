// oxen_amd/csrc/sort_rows.hip -- the stable multi-column row sort (oxh_sort_rows_*): what `sort_df_on_keys`
// (repositories/diffs/join_diff.rs:146-163) does to the joined frame of a keyed diff and `oxen df --sort`
// (core/df/tabular.rs:520-522) to any frame, as a permutation computed on the device from the key columns
// (Arrow: values, offsets, validity bitmaps). The order is stated in include/oxen_hash.h; the key words that
// realise it are sort_keys.hpp's (DESIGN.md §4 "Sort").
//
// The stable radix pass (stable_radix_pass, declared in capi_internal.hpp beside exclusive_scan_u32) moves
// u64 key words with a u32 payload by one 8-bit digit. Tiles of kSortTile elements, one workgroup each:
//   histogram  radix_hist_kernel counts the tile's digits in LDS and writes them to a digit-major
//              [256][tiles] table;
//   scan       exclusive_scan_u32 over that table: entry [d][t] becomes where tile t's elements of digit d go;
//   scatter    radix_scatter_kernel re-reads the tile, finds every element's stable rank among the equal
//              digits of its wave by ballot matching (8 ballots on the digit's bits, mbcnt of the match mask
//              below the lane), adds the waves before it through an LDS prefix over per-wave digit counts,
//              stages the tile in LDS in digit order and stores each digit's run contiguously.
// ELEMENT ORDER INSIDE A TILE -- stability rests on it: element e of a tile is index tile * kSortTile + e;
// wave w owns e in [w * kSortTile / 4, (w + 1) * kSortTile / 4) and takes them 64 at a time, lane l of step k
// holding e = w * kSortTile / 4 + 64 * k + l. Ranks grow with (w, k, l), which is the index order.
//
// One call is MSD refinement over one loop for every kind of key. Places carry a row, a tie-group id (the
// rank of the group among the groups: groups are runs of places) and a cursor (key column, chunk). A round:
//   keys     sort_keys_kernel builds every place's triple (class, word, tail) at its cursor -- a constant
//            past the last key -- as two words: `word`, and `meta` = group << 16 | class << 8 | tail;
//   digits   sort_digits_kernel: one read of both words marks which values each of their bytes takes. A digit
//            with a single value changes nothing and its pass is not launched: the host reads the marks back
//            (with the error word) and runs only the passes that matter, so the ping-pong of the buffers is
//            the host's plain alternation;
//   sort     three stages, each a gather of its word into the order so far and its passes, the payload
//            being the place: meta byte 0 (tail); the word's 8 bytes; meta bytes 1.. (class, then the group
//            id). Stable, so the places end ordered by (group, class, word, tail);
//   regroup  sort_flag_kernel flags the places where (group, class, word, tail) changes, exclusive_scan_u32
//            turns the flags into the new group ids, sort_apply_kernel writes the new places and advances
//            the cursors -- a full 8-byte chunk goes to the next chunk of its cell, everything else to the
//            next key column; the rule reads only the triple, so a group's rows share a cursor -- and
//            counts, per workgroup and with one atomic each, the rows of groups of two or more that have
//            key left, and those that have none (stats3[2] at the end).
// One read-back per round brings the counts and the error word; zero rows with key left ends the loop.
// No lane waits for another lane or workgroup; launches order the steps. Every scattered store is checked
// against the row count first: a violation sets the error word (OXH_ERR_HIP) and nothing wild is written.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "sort_rows_host.hpp"

using namespace oxh::capi;

namespace oxh {

constexpr uint32_t kSortTile = 2048;
constexpr uint32_t kSortPer = kSortTile / 256;   // elements per lane
constexpr uint32_t kSortSpan = kSortTile / 4;    // consecutive elements per wave
// beside kRowErrOffsets, kRowErrValues (columns.hpp)
constexpr unsigned long long kSortErrPlace = 4, kSortErrIndex = 8;
// ctrl words of one call: the error word, the rows of groups >= 2 with key left / with none, then which
// values every digit of the two key words takes (a 256-bit set each)
constexpr int kSortCtrlErr = 0, kSortCtrlMore = 1, kSortCtrlTied = 2, kSortCtrlSeen = 4;
constexpr int kSortWordDigits = 8, kSortMetaDigits = 6, kSortDigits = kSortWordDigits + kSortMetaDigits;
constexpr int kSortCtrlWords = kSortCtrlSeen + 4 * kSortDigits;

uint64_t radix_tiles(uint64_t n) { return (n + kSortTile - 1) / kSortTile; }

__device__ __forceinline__ uint32_t digit_of(uint64_t key, uint32_t shift) { return (uint32_t)(key >> shift) & 255u; }

// ---------------------------------------------------------------- the stable radix pass
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t shift,
                                                         uint64_t ntiles, uint32_t* __restrict__ table) {
    __shared__ uint32_t cnt[256];
    const uint64_t tile = blockIdx.x, base = tile * kSortTile;
    cnt[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kSortPer; ++k) {
        const uint64_t i = base + k * 256 + threadIdx.x;
        if (i < n) atomicAdd(&cnt[digit_of(keys[i], shift)], 1u);
    }
    __syncthreads();
    table[(uint64_t)threadIdx.x * ntiles + tile] = cnt[threadIdx.x];
}

// The lanes of the wave that are live and hold digit d (0 for a lane that is not live). Every lane calls it.
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool live) {
    unsigned long long m = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const unsigned long long v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return live ? m : 0;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The exclusive prefix sum of v over the 256 lanes of the workgroup. Every lane calls it (one barrier after
// the wave sums are written; wave_sum is 4 words of LDS nobody else touches).
__device__ __forceinline__ uint32_t sort_block_scan256(uint32_t v, uint32_t* wave_sum) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= (unsigned)off) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) base += w < wave ? wave_sum[w] : 0;
    return base + incl - v;
}

// scanned: the exclusive scan of the histogram table of this pass (entry [d][tile] = where this tile's
// elements of digit d start in the output).
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t* __restrict__ key_in, const uint32_t* __restrict__ pay_in,
                                                            uint64_t* __restrict__ key_out, uint32_t* __restrict__ pay_out,
                                                            uint64_t n, uint32_t shift, uint64_t ntiles,
                                                            const uint64_t* __restrict__ scanned,
                                                            unsigned long long* __restrict__ ctrl) {
    __shared__ uint32_t cnt[4][256];   // per wave and digit: its elements, then where the wave's start in the digit's run
    __shared__ uint32_t run_at[256];   // where a digit's run starts in the staged tile
    __shared__ uint64_t run_to[256];   // and in the output
    __shared__ uint64_t skey[kSortTile];
    __shared__ uint32_t spay[kSortTile];
    __shared__ uint32_t wave_sum[4];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t tile = blockIdx.x, base = tile * kSortTile;
    const uint32_t count = (uint32_t)(n - base < kSortTile ? n - base : kSortTile);
    unsigned long long bad = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
    __syncthreads();
    uint64_t key[kSortPer];
    uint32_t pay[kSortPer], rank[kSortPer];
    // the rank of every element among the equal digits of its wave's span, in index order
#pragma unroll
    for (uint32_t k = 0; k < kSortPer; ++k) {
        const uint32_t e = wave * kSortSpan + 64 * k + lane;
        const bool live = e < count;
        key[k] = live ? key_in[base + e] : 0;
        pay[k] = live ? pay_in[base + e] : 0;
        const uint32_t d = digit_of(key[k], shift);
        const unsigned long long m = match_digit(d, live);
        const uint32_t below = lanes_below(m);
        const int leader = m ? __ffsll((unsigned long long)m) - 1 : (int)lane;
        uint32_t prior = 0;
        if (live && below == 0) prior = atomicAdd(&cnt[wave][d], (uint32_t)__popcll(m));  // one lane per digit of the step
        prior = (uint32_t)__shfl((int)prior, leader, 64);
        rank[k] = prior + below;
    }
    __syncthreads();
    {   // lane tid owns digit tid: the waves' counts to their exclusive prefix, the digits' totals to the runs
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t c = cnt[w][tid];
            cnt[w][tid] = total;
            total += c;
        }
        run_at[tid] = sort_block_scan256(total, wave_sum);
        run_to[tid] = scanned[(uint64_t)tid * ntiles + tile];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kSortPer; ++k) {
        const uint32_t e = wave * kSortSpan + 64 * k + lane;
        if (e >= count) continue;
        const uint32_t d = digit_of(key[k], shift);
        const uint32_t at = run_at[d] + cnt[wave][d] + rank[k];
        if (at < count) {
            skey[at] = key[k];
            spay[at] = pay[k];
        } else {
            bad |= kSortErrPlace;
        }
    }
    __syncthreads();
    // the staged tile is in digit order: consecutive lanes store consecutive places of a run
#pragma unroll
    for (uint32_t k = 0; k < kSortPer; ++k) {
        const uint32_t e = k * 256 + tid;
        if (e >= count) continue;
        const uint64_t v = skey[e];
        const uint32_t d = digit_of(v, shift);
        const uint64_t to = run_to[d] + (e - run_at[d]);
        if (e >= run_at[d] && to < n) {  // never a store outside the n places
            key_out[to] = v;
            pay_out[to] = spay[e];
        } else {
            bad |= kSortErrPlace;
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kSortCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int stable_radix_pass(const uint64_t* d_key_in, const uint32_t* d_pay_in, uint64_t* d_key_out, uint32_t* d_pay_out, uint64_t n,
                      uint32_t shift, uint32_t* d_table, uint64_t* d_scanned, unsigned long long* d_sums,
                      unsigned long long* d_err, hipStream_t st) {
    const uint64_t ntiles = radix_tiles(n);
    if (!ntiles) return OXH_OK;
    radix_hist_kernel<<<(unsigned)ntiles, 256, 0, st>>>(d_key_in, n, shift, ntiles, d_table);
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(d_table, 256 * ntiles, d_scanned, d_sums, st);
    if (rc) return rc;
    radix_scatter_kernel<<<(unsigned)ntiles, 256, 0, st>>>(d_key_in, d_pay_in, d_key_out, d_pay_out, n, shift, ntiles, d_scanned, d_err);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

// ---------------------------------------------------------------- the rounds
struct SortCol {
    RowCol col;
    uint32_t order, pad;
};

struct SortPlaces {  // what place i holds
    uint32_t *row, *group, *col, *chunk;
};

// The triple of row r's cell of key column sc at `chunk`.
__device__ __forceinline__ sortkeys::Triple cell_triple(const SortCol& sc, uint64_t r, uint64_t chunk, unsigned long long& bad) {
    const RowCol& c = sc.col;
    if (c.validity && !row_bit(c.validity, c.nbit + r)) return sortkeys::null_triple();
    switch (c.kind) {
        case OXH_COL_FIXED1: return sortkeys::fixed_triple(sc.order, 1, c.values[r]);
        case OXH_COL_FIXED4: return sortkeys::fixed_triple(sc.order, 4, ld32u(c.values + 4 * r));
        case OXH_COL_FIXED8: return sortkeys::fixed_triple(sc.order, 8, ld64u(c.values + 8 * r));
        case OXH_COL_BOOL: return sortkeys::bool_triple(row_bit(c.values, c.vbit + r));
        default: break;
    }
    uint64_t start = 0;
    const uint64_t len = row_cell(c, r, start, bad);  // a bad pair of offsets: a cell of length 0
    return sortkeys::bytes_triple(c.values + start, len, chunk);  // reads only inside [start, start + len)
}

__global__ __launch_bounds__(256) void sort_keys_kernel(const SortCol* __restrict__ cols, uint32_t nkeys, uint64_t n, SortPlaces p,
                                                        uint64_t* __restrict__ word, uint64_t* __restrict__ meta,
                                                        uint32_t* __restrict__ place, unsigned long long* __restrict__ ctrl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;  // no barrier and no shuffle below
    unsigned long long bad = 0;
    const uint32_t row = p.row[i], c = p.col[i];
    sortkeys::Triple t = sortkeys::null_triple();  // past the last key: the same for every row
    if (c < nkeys) {
        if (row < n) t = cell_triple(cols[c], row, p.chunk[i], bad);
        else bad |= kSortErrIndex;  // nothing is read through such a row
    }
    word[i] = t.word;
    meta[i] = sortkeys::pack_meta(p.group[i], t);
    place[i] = (uint32_t)i;
    if (bad) __hip_atomic_fetch_or(&ctrl[kSortCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// seen[4 * g + w], bit b: digit g of the key words takes the value 64 * w + b somewhere (g < 8: byte g of
// `word`; else byte g - 8 of `meta`). Grid-stride; a workgroup marks in LDS first (plain stores of 1).
__global__ __launch_bounds__(256) void sort_digits_kernel(const uint64_t* __restrict__ word, const uint64_t* __restrict__ meta,
                                                          uint64_t n, unsigned long long* __restrict__ ctrl) {
    __shared__ uint32_t mark[kSortDigits][256];
    for (int g = 0; g < kSortDigits; ++g) mark[g][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t w = word[i], m = meta[i];
#pragma unroll
        for (int g = 0; g < kSortWordDigits; ++g) mark[g][digit_of(w, 8 * g)] = 1;
#pragma unroll
        for (int g = 0; g < kSortMetaDigits; ++g) mark[kSortWordDigits + g][digit_of(m, 8 * g)] = 1;
    }
    __syncthreads();
    // every lane is here
    for (int g = 0; g < kSortDigits; ++g) {
        const unsigned long long b = __ballot(mark[g][threadIdx.x] != 0);
        if ((threadIdx.x & 63) == 0 && b)
            __hip_atomic_fetch_or(&ctrl[kSortCtrlSeen + 4 * g + (threadIdx.x >> 6)], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// out[i] = src[order[i]]: a stage's key word in the order the stages before it made.
__global__ __launch_bounds__(256) void sort_gather_kernel(const uint64_t* __restrict__ src, const uint32_t* __restrict__ order, uint64_t n,
                                                          uint64_t* __restrict__ out, unsigned long long* __restrict__ ctrl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = order[i];
    if (s >= n) {
        __hip_atomic_fetch_or(&ctrl[kSortCtrlErr], kSortErrIndex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[i] = 0;
        return;
    }
    out[i] = src[s];
}

// flag[j] = 1 where the place sorted to j starts a group: (group, class, word, tail) differs from j - 1's.
__global__ __launch_bounds__(256) void sort_flag_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ word,
                                                        const uint64_t* __restrict__ meta, uint64_t n, uint32_t* __restrict__ flag,
                                                        unsigned long long* __restrict__ ctrl) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = order[j], before = j ? order[j - 1] : 0;
    if (s >= n || before >= n) {
        __hip_atomic_fetch_or(&ctrl[kSortCtrlErr], kSortErrIndex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag[j] = 1;
        return;
    }
    flag[j] = j == 0 || word[s] != word[before] || meta[s] != meta[before];
}

// (the flags are scanned) The new places: row, group id = the groups before it, the advanced cursor; and
// the rows of groups of two or more, by whether they have key left. Every lane reaches the ballots.
__global__ __launch_bounds__(256) void sort_apply_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ meta,
                                                         const uint32_t* __restrict__ flag, const uint64_t* __restrict__ before,
                                                         SortPlaces from, SortPlaces to, uint64_t n, uint32_t nkeys, bool first,
                                                         unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long part[4][2];
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool more = false, tied = false;
    if (j < n) {
        const uint32_t s = order[j];
        if (s >= n) {
            __hip_atomic_fetch_or(&ctrl[kSortCtrlErr], kSortErrIndex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const uint32_t f = flag[j], fnext = j + 1 < n ? flag[j + 1] : 1;
            const uint64_t m = meta[s];
            // round 1's places are the rows themselves at the first key: nothing to gather then
            uint32_t col = first ? 0 : from.col[s], chunk = first ? 0 : from.chunk[s];
            if (col < nkeys) {
                if (sortkeys::meta_class(m) == sortkeys::kClassPresent && sortkeys::meta_tail(m) == sortkeys::kChunk) {
                    chunk += 1;
                } else {
                    col += 1;
                    chunk = 0;
                }
            }
            to.row[j] = first ? s : from.row[s];
            to.group[j] = (uint32_t)(before[j] + f - 1);  // flag[0] is 1: never below 0
            to.col[j] = col;
            to.chunk[j] = chunk;
            const bool shared = !(f && fnext);  // a group of two or more
            more = shared && col < nkeys;
            tied = shared && col >= nkeys;
        }
    }
    const unsigned long long nmore = __popcll(__ballot(more)), ntied = __popcll(__ballot(tied));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][0] = nmore, part[threadIdx.x >> 6][1] = ntied;
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (sum) atomicAdd(&ctrl[kSortCtrlMore + threadIdx.x], sum);
    }
}

// place i holds row i, group 0, the cursor at the first key
__global__ __launch_bounds__(256) void sort_init_kernel(SortPlaces p, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    p.row[i] = (uint32_t)i;
    p.group[i] = 0;
    p.col[i] = 0;
    p.chunk[i] = 0;
}

}  // namespace oxh

namespace {

using oxh::cols::is_bytes;
namespace sortrows = oxh::sortrows;

unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }
unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 2048); }
uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

int sort_error(unsigned long long e) {
    if (!e) return OXH_OK;
    if (e & (oxh::kSortErrPlace | oxh::kSortErrIndex))
        return fail(OXH_ERR_HIP, "sort rows: a place outside the rows (the keys changed during the call?); no result");
    if (e & oxh::kRowErrOffsets) return fail(OXH_ERR_INVALID, "sort rows: a byte column's offsets decrease or are negative");
    return fail(OXH_ERR_INVALID, "sort rows: a byte column has bytes but no values");
}

// One call over device-resident key columns; d_perm filled and the stream drained on return. The small block
// holds [SortCol nkeys | ctrl], on the device and pinned; everything row-shaped is leased from scratch.hpp:
// two sets of places (16 B each), the two key words (16 B), the order and the key word of the passes, twice
// (24 B), the flags and their scan (12 B) -- 84 B per row -- and the histogram table with its scan (12 B per
// 8 rows).
int sort_rows_run(const sortrows::Args& a, const void* const* d_values, const void* const* d_offsets,
                  const uint8_t* const* d_validity, const uint64_t* bits, uint32_t* d_perm, hipStream_t st) {
    using namespace oxh;
    const uint64_t n = a.nrows, ntiles = radix_tiles(n), ntable = 256 * ntiles;
    const size_t ctrl_at = (a.nkeys * sizeof(SortCol) + 63) & ~(size_t)63, ctrl_bytes = kSortCtrlWords * 8;
    CallBlock block;
    int rc = block.make(ctrl_at + ctrl_bytes, "sort rows", st);
    if (rc) return rc;
    SortCol* h_cols = (SortCol*)block.h;
    for (uint32_t c = 0; c < a.nkeys; ++c) {
        h_cols[c].col.values = (const uint8_t*)d_values[c];
        h_cols[c].col.offsets = is_bytes(a.kinds[c]) ? (const uint8_t*)d_offsets[c] : nullptr;
        h_cols[c].col.validity = d_validity[c];
        h_cols[c].col.vbit = bits[2 * c];
        h_cols[c].col.nbit = bits[2 * c + 1];
        h_cols[c].col.kind = a.kinds[c];
        h_cols[c].order = a.orders[c];
    }
    const SortCol* d_cols = (const SortCol*)block.d;
    unsigned long long* d_ctrl = (unsigned long long*)(block.d + ctrl_at);
    const unsigned long long* h_ctrl = (const unsigned long long*)(block.h + ctrl_at);

    const uint64_t b4 = align256(n * 4), b8 = align256(n * 8);
    const uint64_t nsums = std::max(scan_tiles(ntable), scan_tiles(n)) + 1;
    const uint64_t total = 8 * b4 + 2 * b8 + 2 * b4 + 2 * b8 + b4 + b8 + align256(ntable * 4) + align256(ntable * 8) + align256(nsums * 8);
    ScratchLease lease(st);  // ends (and waits for the stream) before the block is freed
    void* base = nullptr;
    if (lease.get(total, &base) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "sort rows: " + std::to_string(total) + " B of places and key words");
    }
    uint8_t* at = (uint8_t*)base;
    auto carve = [&](uint64_t bytes) {
        uint8_t* here = at;
        at += bytes;
        return here;
    };
    SortPlaces places[2];
    for (SortPlaces& p : places) {
        p.row = (uint32_t*)carve(b4), p.group = (uint32_t*)carve(b4);
        p.col = (uint32_t*)carve(b4), p.chunk = (uint32_t*)carve(b4);
    }
    uint64_t *word = (uint64_t*)carve(b8), *meta = (uint64_t*)carve(b8);
    uint32_t* order[2] = {(uint32_t*)carve(b4), (uint32_t*)carve(b4)};
    uint64_t* keys[2] = {(uint64_t*)carve(b8), (uint64_t*)carve(b8)};
    uint32_t* flag = (uint32_t*)carve(b4);
    uint64_t* flag_scan = (uint64_t*)carve(b8);
    uint32_t* table = (uint32_t*)carve(align256(ntable * 4));
    uint64_t* table_scan = (uint64_t*)carve(align256(ntable * 8));
    unsigned long long* sums = (unsigned long long*)carve(align256(nsums * 8));

    HIP_TRY(hipMemcpyAsync(block.d, block.h, ctrl_at, hipMemcpyHostToDevice, st));
    sort_init_kernel<<<grid_for(n), 256, 0, st>>>(places[0], n);
    HIP_TRY(hipGetLastError());
    auto read_ctrl = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(block.h + ctrl_at, d_ctrl, ctrl_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return sort_error(h_ctrl[kSortCtrlErr]);
    };
    uint64_t rounds = 0, passes = 0, tied = 0;
    int cur = 0;  // the places of this round
    for (;;) {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, ctrl_bytes, st));
        sort_keys_kernel<<<grid_for(n), 256, 0, st>>>(d_cols, a.nkeys, n, places[cur], word, meta, order[0], d_ctrl);
        HIP_TRY(hipGetLastError());
        sort_digits_kernel<<<stride_grid(n), 256, 0, st>>>(word, meta, n, d_ctrl);
        HIP_TRY(hipGetLastError());
        if ((rc = read_ctrl())) return rc;
        auto active = [&](int g) {  // does digit g take more than one value?
            const unsigned long long* s = h_ctrl + kSortCtrlSeen + 4 * g;
            return __builtin_popcountll(s[0]) + __builtin_popcountll(s[1]) + __builtin_popcountll(s[2]) + __builtin_popcountll(s[3]) > 1;
        };
        // the three stages: (source word, first digit, digits); the order so far is order[oc], the identity at first
        struct Stage {
            const uint64_t* src;
            int seen0, first, count;
        } const stages[3] = {{meta, kSortWordDigits, 0, 1}, {word, 0, 0, kSortWordDigits}, {meta, kSortWordDigits, 1, kSortMetaDigits - 1}};
        int oc = 0;
        bool identity = true;
        for (const Stage& s : stages) {
            const uint64_t* in = nullptr;
            int kc = 0;  // the key buffer the next pass writes
            for (int g = s.first; g < s.first + s.count; ++g) {
                if (!active(s.seen0 + g)) continue;
                if (!in) {
                    if (identity) {
                        in = s.src;
                    } else {
                        sort_gather_kernel<<<grid_for(n), 256, 0, st>>>(s.src, order[oc], n, keys[0], d_ctrl);
                        HIP_TRY(hipGetLastError());
                        in = keys[0], kc = 1;
                    }
                }
                if ((rc = stable_radix_pass(in, order[oc], keys[kc], order[oc ^ 1], n, 8 * g, table, table_scan, sums, d_ctrl, st))) return rc;
                in = keys[kc], kc ^= 1, oc ^= 1;
                identity = false;
                passes += 1;
            }
        }
        sort_flag_kernel<<<grid_for(n), 256, 0, st>>>(order[oc], word, meta, n, flag, d_ctrl);
        HIP_TRY(hipGetLastError());
        if ((rc = exclusive_scan_u32(flag, n, flag_scan, sums, st))) return rc;
        sort_apply_kernel<<<grid_for(n), 256, 0, st>>>(order[oc], meta, flag, flag_scan, places[cur], places[cur ^ 1], n, a.nkeys, rounds == 0, d_ctrl);
        HIP_TRY(hipGetLastError());
        if ((rc = read_ctrl())) return rc;  // the round's one read-back of its result
        cur ^= 1;
        rounds += 1;
        tied = h_ctrl[kSortCtrlTied];
        STEP("sort rows: round %llu, %llu passes so far, %llu rows still tied with key left", (unsigned long long)rounds,
             (unsigned long long)passes, (unsigned long long)h_ctrl[kSortCtrlMore]);
        if (!h_ctrl[kSortCtrlMore]) break;
    }
    HIP_TRY(hipMemcpyAsync(d_perm, places[cur].row, n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    a.stats3[0] = rounds, a.stats3[1] = passes, a.stats3[2] = tied;
    return OXH_OK;
}

// What both forms do before they need a device. `done`: no rows, nothing left to do.
int sort_enter(oxh_ctx* ctx, const sortrows::Args& a, bool host, bool& done) {
    done = false;
    const std::string what = sortrows::argument_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "sort rows: " + what);
    if (a.nrows == 0) {
        a.stats3[0] = a.stats3[1] = a.stats3[2] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

}  // namespace

extern "C" {

int oxh_sort_rows_device(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* d_values,
                         const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                         const uint32_t* orders, uint32_t* d_perm, uint64_t* stats3, void* stream) {
    const sortrows::Args a{nrows, nkeys, kinds, d_values, d_offsets, d_validity, bit_offsets, orders, d_perm, stats3};
    bool done = false;
    int rc = sort_enter(ctx, a, false, done);
    if (rc || done) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = sort_rows_run(a, d_values, d_offsets, d_validity, bit_offsets, d_perm, st);
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

int oxh_sort_rows_host(oxh_ctx* ctx, uint64_t nrows, uint32_t nkeys, const uint32_t* kinds, const void* const* values,
                       const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                       const uint32_t* orders, uint32_t* perm, uint64_t* stats3) {
    const sortrows::Args a{nrows, nkeys, kinds, values, offsets, validity, bit_offsets, orders, perm, stats3};
    bool done = false;
    int rc = sort_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // One device block: the permutation, then for every key column only what its rows name (columns.hpp).
    const sortrows::HostPlan plan(a);
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, plan.staging.total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "sort rows: " + std::to_string(plan.staging.total) + " B for the key columns on the device");
    }
    oxh::poison_device(d_block, plan.staging.total + 16, st);
    uint64_t stats[3] = {0, 0, 0};
    std::vector<uint32_t> out;
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
        sortrows::Args d = a;
        d.stats3 = stats;
        int r = sort_rows_run(d, d_values.data(), d_offsets.data(), d_validity.data(), bits.data(), (uint32_t*)d_block, st);
        if (r) return r;
        out.resize(nrows);  // perm stays untouched unless everything succeeded
        HIP_TRY(hipMemcpyAsync(out.data(), d_block, nrows * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    if (rc) return rc;
    memcpy(perm, out.data(), nrows * 4);
    memcpy(stats3, stats, sizeof stats);
    return OXH_OK;
}

}  // extern "C"
