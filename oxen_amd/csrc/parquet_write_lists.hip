// oxen_amd/csrc/parquet_write_lists.hip -- the LIST columns of the Parquet writer (oxh_write_parquet_lists_*; the
// format is stated in include/oxen_hash.h "Parquet", DESIGN.md §4 "Parquet"): Arrow lists of numbers to repetition and
// definition levels and compacted PLAIN values, the inverse of parquet_lists.hip. The work is split by LEVEL ENTRIES,
// not by rows -- one entry per element, one per empty or null list -- because a row may hold any number of them:
//   count    pql_count_kernel, a lane per row: 1 for a null or empty list, else its length, the pair of offsets
//            checked first. The device-wide exclusive_scan_u32 gives entry0[row], the entries in front of a row;
//            entry0[nrows] is the column's total and comes down, since it sizes what follows;
//   levels   pql_levels_kernel: a wave takes a run of kPqlRunWords consecutive 64-entry words of the column's entry
//            space. A lane finds its entry's row by a search of entry0 -- over all rows once per run, then over the at
//            most 64 rows behind the previous word's last row (every row has an entry), and not at all when the whole
//            word lies in one row, the embedding case -- and derives rep (not the row's first entry), def (0 null list,
//            1 empty, 2 null element, 3 value) and its element. Four ballots leave as 64-bit words: rep, def bit 0, def
//            bit 1, value; the value word's popcount is kept and scanned, so every word knows the values in front of
//            it. Half a byte of scratch per entry, and 20 bytes per word for the counts and ranks;
//   tiles    pql_tiles_kernel, a wave per 1 024-row tile: the tile's entries and values (the ranks at its two boundary
//            entries) and its lists that are not null, into the tile table the planner reads (parquet_host.hpp);
//   emit     pql_emit_kernel, a wave per (page, block of 4 096 entries) from a host-built list. A page starts at any
//            bit of a global word: each lane builds one page-local word by a funnel shift of two neighbouring global
//            words. 8 bytes of repetition bits a lane, 16 of definition bits with the two planes interleaved, staged
//            in the wave's LDS at the destination's misalignment and stored as aligned 16-byte blocks; a stream that is
//            one RLE run costs nothing beyond its head, which the block 0 of a page copies from the plan. Values: a
//            page whose values equal its entries holds one contiguous span of elements, and a block is a straight
//            shifted copy (pqw_copy_span: the embedding case). Else 1 024 entries at a time: an entry with the value bit
//            finds its row as above, loads values[element] and puts it at its rank -- the word's base, the popcounts
//            in front, mbcnt in the ballot -- in LDS, and the span leaves as aligned blocks.
// Elements under a null list are never read. Every byte has one writer, every store is checked against the page's own
// sizes first, and what is inconsistent (columns that change during the call) sets the error word. No workgroup waits
// for another; launches order the steps. Row, word and item kernels keep a launch cap and stride beyond it.
#include <chrono>

#include "parquet_device.hpp"

using namespace oxh::capi;
namespace pq = oxh::parquet;

namespace oxh {

constexpr uint32_t kPqlRunWords = 32;   // the consecutive words of one wave's run in the levels kernel
constexpr unsigned kPqlTileGroups = 64;  // the tiles kernel's cap: a wave per tile is little work

// Row r's list: whether it is not null, and its elements [start, start + len). A pair of offsets that is negative or
// decreases, a list of more than INT32_MAX elements and elements without values are an empty list and an error bit.
__device__ __forceinline__ bool pql_row(const PqListCol& L, uint64_t r, uint64_t& start, uint64_t& len, unsigned long long& bad) {
    start = len = 0;
    if (L.c.validity && !row_bit(L.c.validity, L.c.nbit + r)) return false;
    int64_t s, e;
    if (L.wide) {
        s = ((const int64_t*)L.c.offsets)[r], e = ((const int64_t*)L.c.offsets)[r + 1];
    } else {
        s = ((const int32_t*)L.c.offsets)[r], e = ((const int32_t*)L.c.offsets)[r + 1];
    }
    if (s < 0 || e < s) return bad |= kPqErrListOffsets, true;  // never a read through such a pair
    if ((uint64_t)(e - s) > pq::kMaxPage) return bad |= kPqErrListLong, true;
    if (e > s && (!L.c.values || (uint64_t)s < L.elem_lo)) return bad |= kPqErrListValues, true;
    start = (uint64_t)s, len = (uint64_t)(e - s);
    return true;
}

// The row r in [lo, hi] with entry0[r] <= e < entry0[r + 1]; entry0 rises strictly, e lies in the range's entries.
__device__ __forceinline__ uint64_t pql_row_of(const uint64_t* __restrict__ entry0, uint64_t lo, uint64_t hi, uint64_t e) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (entry0[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The rows of a word's live entries, whose first entry's row is at least `first` (uniform) and at most `last`; on
// return `first` is the row of the word's last live entry, where the next word's search starts.
__device__ __forceinline__ uint64_t pql_word_rows(const uint64_t* __restrict__ entry0, uint64_t& first, uint64_t last, uint64_t e, bool live,
                                                  unsigned long long live_mask) {
    const int top = 63 - __builtin_clzll(live_mask);  // live_mask != 0
    const uint64_t e_top = (uint64_t)__shfl((long long)e, top, 64);
    uint64_t row = first;
    if (entry0[first + 1] <= e_top) {  // uniform: the word spans rows, at most 64 of them
        const uint64_t hi = last - first < 64 ? last : first + 64;
        if (live) row = pql_row_of(entry0, first, hi, e);
    }
    first = (uint64_t)__shfl((long long)row, top, 64);
    return row;
}

__device__ __forceinline__ bool pql_child_valid(const PqListCol& L, uint64_t elem) {
    return !L.child || row_bit(L.child, L.cbit + (elem - L.elem_lo));
}

// ---------------------------------------------------------------- count
__global__ __launch_bounds__(256) void pql_count_kernel(const PqListCol L, uint64_t nrows, unsigned long long* __restrict__ ctrl) {
    unsigned long long bad = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r <= nrows; r += (uint64_t)gridDim.x * 256) {
        uint64_t start, len = 0;
        if (r < nrows) pql_row(L, r, start, len, bad);
        L.count[r] = r == nrows ? 0u : len ? (uint32_t)len : 1u;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- levels
__global__ __launch_bounds__(256) void pql_levels_kernel(const PqListCol L, uint64_t nrows, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t nruns = (L.nwords + kPqlRunWords - 1) / kPqlRunWords, nwaves = (uint64_t)gridDim.x * 4;
    unsigned long long bad = 0;
    for (uint64_t run = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); run < nruns; run += nwaves) {  // uniform in the wave
        const uint64_t w0 = run * kPqlRunWords, w1 = w0 + kPqlRunWords < L.nwords ? w0 + kPqlRunWords : L.nwords;
        uint64_t first = pql_row_of(L.entry0, 0, nrows - 1, 64 * w0);  // uniform: every lane takes the same steps
        for (uint64_t w = w0; w < w1; ++w) {
            const uint64_t e = 64 * w + lane;
            const bool live = e < L.total;
            const uint64_t row = pql_word_rows(L.entry0, first, nrows - 1, e, live, __ballot(live));
            uint32_t rep = 0, def = 0;
            if (live) {
                uint64_t start, len;
                const uint64_t at = e - L.entry0[row];
                const bool present = pql_row(L, row, start, len, bad);
                rep = at != 0;
                if (at >= (len ? len : 1)) bad |= kPqErrPlace, def = 0;  // the offsets are not what was counted
                else def = !present ? 0 : !len ? 1 : pql_child_valid(L, start + at) ? 3 : 2;
            }
            const unsigned long long b0 = __ballot(rep != 0), b1 = __ballot(def & 1), b2 = __ballot(def & 2), b3 = __ballot(def == 3);
            if (lane == 0) L.words[0][w] = b0;
            if (lane == 1) L.words[1][w] = b1;
            if (lane == 2) L.words[2][w] = b2;
            if (lane == 3) L.words[3][w] = b3;
            if (lane == 4) L.vcount[w] = (uint32_t)__popcll(b3);
            if (lane == 5 && w + 1 == L.nwords) L.vcount[L.nwords] = 0;
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The values in front of entry e of the column (e <= total).
__device__ __forceinline__ uint64_t pql_rank(const PqListCol& L, uint64_t e) {
    const uint64_t w = e >> 6;
    if (w >= L.nwords) return L.vbase[L.nwords];
    return L.vbase[w] + (uint64_t)__popcll(L.words[3][w] & ((1ull << (e & 63)) - 1));
}

// ---------------------------------------------------------------- tiles
__global__ __launch_bounds__(256) void pql_tiles_kernel(const PqListCol L, uint64_t nrows, uint64_t ntiles, uint32_t ncols, pq::Tile* __restrict__ tiles) {
    const unsigned lane = threadIdx.x & 63;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += (uint64_t)gridDim.x * 4) {  // uniform in the wave
        const uint64_t r0 = t * pq::kTileRows, r1 = nrows - r0 < pq::kTileRows ? nrows : r0 + pq::kTileRows;
        uint32_t valid = 0;
        for (uint64_t r = r0; r < r1; r += 64) valid += (uint32_t)__popcll(__ballot(r + lane < r1 && pqw_present(L.c, r + lane)));
        const uint64_t e0 = L.entry0[r0], e1 = L.entry0[r1];
        pq::Tile tl{};
        tl.value_bytes = (pql_rank(L, e1) - pql_rank(L, e0)) * L.width, tl.min = e1 - e0, tl.valid = valid;
        if (lane == 0) tiles[t * ncols + L.col] = tl;
    }
}

// ---------------------------------------------------------------- emit
// The 64 bits from bit g of a plane on (g < 64 * nwords), the first nbits of them kept.
__device__ __forceinline__ uint64_t pql_funnel(const uint64_t* __restrict__ plane, uint64_t nwords, uint64_t g, uint32_t nbits) {
    const uint64_t w = g >> 6;
    const uint32_t sh = (uint32_t)(g & 63);
    uint64_t v = plane[w] >> sh;
    if (sh && w + 1 < nwords) v |= plane[w + 1] << (64 - sh);
    return nbits < 64 ? v & ((1ull << nbits) - 1) : v;
}

// The 32 bits of x at the even bits of a word.
__device__ __forceinline__ uint64_t pql_spread(uint32_t x) {
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    return (v | (v << 1)) & 0x5555555555555555ull;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void pql_emit_kernel(const PqListCol L, const PqlItem* __restrict__ items, uint64_t nitems,
                                                                                              const PqEmit e, unsigned long long* __restrict__ ctrl) {
    __shared__ __attribute__((aligned(16))) uint8_t spans[4][kPqSpanLds + 16];
    const unsigned lane = threadIdx.x & 63;
    uint8_t* const stage = spans[threadIdx.x >> 6];
    unsigned long long bad = 0;
    for (uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < nitems; item += (uint64_t)gridDim.x * 4) {  // uniform in the wave
        const PqlItem it = items[item];
        if (it.page >= e.npages) {
            bad |= kPqErrPlace;
            continue;
        }
        const pq::Page pg = e.pages[it.page];
        const uint64_t n_all = pg.entries, e_lo = (uint64_t)it.block * kPqlBlockEntries;
        const bool rep_rle = n_all == pg.rows, def_rle = n_all == pg.nvalid;
        const uint64_t rep_bytes = rep_rle ? 0 : (n_all + 7) / 8, def_bytes = def_rle ? 0 : (n_all + 7) / 8 * 2;
        if (pg.col != L.col || !pg.rows || pg.rows > n_all || pg.nvalid > n_all || e_lo >= n_all || pg.entry0 + n_all > L.total ||
            rep_bytes + pg.def_head_len + def_bytes != pg.level_bytes || (uint64_t)pg.nvalid * L.width != pg.values_bytes) {
            bad |= kPqErrPlace;
            continue;
        }
        const uint64_t n = n_all - e_lo < kPqlBlockEntries ? n_all - e_lo : kPqlBlockEntries;
        uint8_t* const page_out = e.out + pg.file_at;
        uint8_t* const rep_out = page_out + pg.head_len;
        uint8_t* const def_out = rep_out + rep_bytes + pg.def_head_len;
        uint8_t* const vals = page_out + pg.head_len + pg.level_bytes;
        if (it.block == 0) {
            copy_span_wave(page_out, e.blob + pg.head_src, pg.head_len, lane);
            copy_span_wave(rep_out + rep_bytes, e.blob + pg.head_src + pg.head_len, pg.def_head_len, lane);
        }
        // this lane's page-local word: the entries e_lo + 64 * lane on, `nbits` of them inside the page
        const uint64_t mine = e_lo + 64ull * lane;
        const uint32_t nbits = mine >= e_lo + n ? 0u : e_lo + n - mine < 64 ? (uint32_t)(e_lo + n - mine) : 64u;
        const uint64_t g = pg.entry0 + mine;
        if (!rep_rle) {  // 512 bytes of repetition bits a block
            uint8_t* const d = rep_out + 512ull * it.block;
            const uint64_t left = rep_bytes - 512ull * it.block, cnt = left < 512 ? left : 512;
            const uint64_t v = nbits ? pql_funnel(L.words[0], L.nwords, g, nbits) : 0;
            __builtin_memcpy(stage + ((uintptr_t)d & 15) + 8 * lane, &v, 8);
            pqw_wave_lds_order();
            pqw_store_span(d, cnt, stage, lane);
            pqw_wave_lds_order();
        }
        if (!def_rle) {  // 1 024 bytes of definition levels a block: entry i at bits 2 i and 2 i + 1
            uint8_t* const d = def_out + 1024ull * it.block;
            const uint64_t left = def_bytes - 1024ull * it.block, cnt = left < 1024 ? left : 1024;
            const uint64_t d0 = nbits ? pql_funnel(L.words[1], L.nwords, g, nbits) : 0, d1 = nbits ? pql_funnel(L.words[2], L.nwords, g, nbits) : 0;
            const uint64_t v[2] = {pql_spread((uint32_t)d0) | (pql_spread((uint32_t)d1) << 1), pql_spread((uint32_t)(d0 >> 32)) | (pql_spread((uint32_t)(d1 >> 32)) << 1)};
            __builtin_memcpy(stage + ((uintptr_t)d & 15) + 16 * lane, v, 16);
            pqw_wave_lds_order();
            pqw_store_span(d, cnt, stage, lane);
            pqw_wave_lds_order();
        }
        if (!pg.nvalid) continue;
        if (def_rle) {
            // every entry is a value: no null or empty list, so the page's elements are one span from its first row's
            // offset, and the block is a straight shifted copy
            uint64_t start, len, end_start, end_len;
            pql_row(L, pg.row0, start, len, bad);
            pql_row(L, pg.row0 + pg.rows - 1, end_start, end_len, bad);
            if (end_start + end_len - start != n_all) {  // uniform
                bad |= kPqErrPlace;
                continue;
            }
            pqw_copy_span(vals + L.width * e_lo, L.c.values + L.width * (start - L.elem_lo + e_lo), L.width * n, lane);
            continue;
        }
        const uint64_t vword = nbits ? pql_funnel(L.words[3], L.nwords, g, nbits) : 0;
        const uint64_t last_row = pg.row0 + pg.rows - 1;
        for (uint32_t sub = 0; sub < kPqlBlockEntries / 1024 && 1024ull * sub < n; ++sub) {  // 1 024 entries: at most 8 KiB of values
            const uint64_t s_lo = e_lo + 1024ull * sub, g0 = pg.entry0 + s_lo;
            const uint64_t rank0 = pql_rank(L, g0) - pg.value0;
            if (rank0 > pg.nvalid) {  // uniform: the plan's value base is not the words'
                bad |= kPqErrPlace;
                break;
            }
            uint8_t* const d = vals + L.width * rank0;
            const uint32_t shift = (uint32_t)((uintptr_t)d & 15);
            uint64_t first = pql_row_of(L.entry0, pg.row0, last_row, g0);  // uniform
            uint32_t cnt = 0;
            for (uint32_t k = 0; k < 16 && s_lo + 64ull * k < e_lo + n; ++k) {
                const uint64_t wk = (uint64_t)__shfl((long long)vword, (int)(16 * sub + k), 64);
                const uint64_t en = g0 + 64ull * k + lane;
                const bool live = s_lo + 64ull * k + lane < e_lo + n;
                const uint64_t row = pql_word_rows(L.entry0, first, last_row, en, live, __ballot(live));
                if ((wk >> lane) & 1) {
                    uint64_t start, len;
                    pql_row(L, row, start, len, bad);
                    const uint64_t at = en - L.entry0[row];
                    if (at < len) {  // else the offsets are not what was counted: the place keeps the stage's bytes
                        const uint8_t* src = L.c.values + L.width * (start + at - L.elem_lo);
                        uint8_t* to = stage + shift + L.width * (cnt + pqw_below(wk));
                        if (L.width == 8) {
                            const uint64_t v = ld64u(src);
                            __builtin_memcpy(to, &v, 8);
                        } else {
                            const uint32_t v = ld32u(src);
                            __builtin_memcpy(to, &v, 4);
                        }
                    } else {
                        bad |= kPqErrPlace;
                    }
                }
                cnt += (uint32_t)__popcll(wk);
            }
            pqw_wave_lds_order();  // the span is assembled
            if (rank0 + cnt <= pg.nvalid)
                pqw_store_span(d, (uint64_t)L.width * cnt, stage, lane);
            else
                bad |= kPqErrPlace;
            pqw_wave_lds_order();  // the span is stored: the next one may overwrite it
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- the call's steps
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~255ull; }
}  // namespace

namespace {
double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

// OXH_TRACE (env.hpp, read per call): events around the steps of the last list column and a host clock around the
// allocations and the wait for the totals; emit() waits for the last event and leaves one line on stderr, the
// destructor one for the two frees. Without it nothing is recorded.
void PqLists::mark(int k, hipStream_t st) {
    if (!trace) return;
    if (!ev[k]) (void)hipEventCreate(&ev[k]);
    (void)hipEventRecord(ev[k], st);
}

PqLists::~PqLists() {
    const double t0 = trace ? wall_ms() : 0;
    if (d_rows) (void)hipFree(d_rows);
    if (d_words) (void)hipFree(d_words);
    if (trace && d_words) fprintf(stderr, "PQL_FREE {\"free_ms\": %.3f}\n", wall_ms() - t0);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

int PqLists::measure(const PqArgs& args, const uint32_t* types, const PqCol* h_cols, const uint8_t* const* d_child, const uint64_t* child_bits,
                     const uint64_t* elem_lo, pq::Tile* d_tiles, unsigned long long* d_ctrl, unsigned long long* h_ctrl, hipStream_t st) {
    const uint64_t n = args.nrows;
    ntiles = args.ntiles;
    for (uint32_t c = 0; c < args.ncols; ++c) {
        if (!pq::is_list(types[c])) continue;
        PqListCol L{};
        L.c = h_cols[c].c;
        L.child = d_child ? d_child[c] : nullptr, L.cbit = d_child && child_bits ? child_bits[c] : 0, L.elem_lo = elem_lo ? elem_lo[c] : 0;
        L.col = c, L.width = pq::element_width(types[c]), L.wide = pq::list_offset_width(types[c]) == 8;
        cols.push_back(L);
    }
    if (cols.empty() || !n) return OXH_OK;
    trace = env::trace();
    double t0 = trace ? wall_ms() : 0;
    // per column over the rows: [count u32 | entry0 u64 | the scan's sums]
    const uint64_t count_bytes = up256((n + 1) * 4), entry_bytes = up256((n + 1) * 8), sums_bytes = up256((scan_tiles(n + 1) + 1) * 8);
    const uint64_t per_col = count_bytes + entry_bytes + sums_bytes, rows_total = per_col * cols.size();
    if (hipMalloc(&d_rows, rows_total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet write: " + std::to_string(rows_total) + " B for the list columns' entry counts");
    }
    poison_device(d_rows, rows_total, st);
    if (trace) host_ms[0] = wall_ms() - t0;
    mark(0, st);
    const unsigned row_grid = (unsigned)std::min<uint64_t>((n + 256) / 256, kPqMaxGroups);
    std::vector<uint64_t> totals(cols.size());
    for (size_t k = 0; k < cols.size(); ++k) {
        PqListCol& L = cols[k];
        uint8_t* base = d_rows + k * per_col;
        L.count = (uint32_t*)base, L.entry0 = (uint64_t*)(base + count_bytes);
        pql_count_kernel<<<row_grid, 256, 0, st>>>(L, n, d_ctrl);
        HIP_TRY(hipGetLastError());
        const int rc = exclusive_scan_u32(L.count, n + 1, L.entry0, (unsigned long long*)(base + count_bytes + entry_bytes), st);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(&totals[k], L.entry0 + n, 8, hipMemcpyDeviceToHost, st));
    }
    mark(1, st);
    HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
    t0 = trace ? wall_ms() : 0;
    HIP_TRY(hipStreamSynchronize(st));
    if (trace) host_ms[1] = wall_ms() - t0;
    if (h_ctrl[kPqErr]) return OXH_OK;  // the caller names the cause; nothing below reads through a bad pair, but nothing below is needed
    // per column over the words: [4 planes u64 | vcount u32 | vbase u64 | the scan's sums | the emit's items]
    std::vector<uint64_t> at(cols.size() + 1, 0);
    items_at.assign(cols.size(), 0);
    for (size_t k = 0; k < cols.size(); ++k) {
        PqListCol& L = cols[k];
        L.total = totals[k], L.nwords = (L.total + 63) / 64;
        if (L.total < n) return fail(OXH_ERR_HIP, "parquet write: a list column counts fewer entries than rows");
        const uint64_t planes = 4 * up256(L.nwords * 8), vcount = up256((L.nwords + 1) * 4), vbase = up256((L.nwords + 1) * 8);
        const uint64_t sums = up256((scan_tiles(L.nwords + 1) + 1) * 8);
        items_at[k] = at[k] + planes + vcount + vbase + sums;
        at[k + 1] = items_at[k] + up256((L.total / kPqlBlockEntries + args.ntiles + 1) * sizeof(PqlItem));  // a page holds a tile at least
    }
    t0 = trace ? wall_ms() : 0;
    if (hipMalloc(&d_words, at.back()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet write: " + std::to_string(at.back()) + " B for the list columns' level words");
    }
    poison_device(d_words, at.back(), st);
    if (trace) host_ms[2] = wall_ms() - t0;
    for (size_t k = 0; k < cols.size(); ++k) {
        PqListCol& L = cols[k];
        uint8_t* base = d_words + at[k];
        const uint64_t plane = up256(L.nwords * 8);
        for (int j = 0; j < 4; ++j) L.words[j] = (uint64_t*)(base + j * plane);
        L.vcount = (uint32_t*)(base + 4 * plane);
        L.vbase = (uint64_t*)(base + 4 * plane + up256((L.nwords + 1) * 4));
        unsigned long long* sums = (unsigned long long*)((uint8_t*)L.vbase + up256((L.nwords + 1) * 8));
        const uint64_t nruns = (L.nwords + kPqlRunWords - 1) / kPqlRunWords;
        mark(2, st);
        pql_levels_kernel<<<(unsigned)std::min<uint64_t>((nruns + 3) / 4, kPqMaxGroups), 256, 0, st>>>(L, n, d_ctrl);
        HIP_TRY(hipGetLastError());
        mark(3, st);
        const int rc = exclusive_scan_u32(L.vcount, L.nwords + 1, L.vbase, sums, st);
        if (rc) return rc;
        mark(4, st);
        pql_tiles_kernel<<<(unsigned)std::min<uint64_t>((args.ntiles + 3) / 4, kPqlTileGroups), 256, 0, st>>>(L, n, args.ntiles, args.ncols, d_tiles);
        HIP_TRY(hipGetLastError());
        mark(5, st);
    }
    return OXH_OK;
}

int PqLists::emit(const PqEmit& em, const pq::Plan& plan, unsigned long long* d_ctrl, hipStream_t st) {
    if (!d_words) return OXH_OK;
    items.clear();
    std::vector<uint64_t> first(cols.size() + 1, 0);
    for (size_t k = 0; k < cols.size(); ++k) {
        for (size_t p = 0; p < plan.pages.size(); ++p) {
            const pq::Page& pg = plan.pages[p];
            if (pg.col != cols[k].col) continue;
            for (uint64_t b = 0; b * kPqlBlockEntries < pg.entries; ++b) items.push_back(PqlItem{(uint32_t)p, (uint32_t)b});
        }
        first[k + 1] = items.size();
        if (first[k + 1] - first[k] > cols[k].total / kPqlBlockEntries + ntiles + 1)  // measure()'s room
            return fail(OXH_ERR_HIP, "parquet write: the list pages outgrew their room");
    }
    for (size_t k = 0; k < cols.size(); ++k) {
        const uint64_t cnt = first[k + 1] - first[k];
        if (!cnt) continue;
        PqlItem* d_items = (PqlItem*)(d_words + items_at[k]);
        HIP_TRY(hipMemcpyAsync(d_items, items.data() + first[k], cnt * sizeof(PqlItem), hipMemcpyHostToDevice, st));
        mark(6, st);
        pql_emit_kernel<<<(unsigned)std::min<uint64_t>((cnt + 3) / 4, kPqMaxGroups), 256, 0, st>>>(cols[k], d_items, cnt, em, d_ctrl);
        HIP_TRY(hipGetLastError());
        mark(7, st);
    }
    if (trace && ev[7]) {
        // plan_ms: from the tiles kernel's end to the last emit kernel's start -- the tile table coming down, the
        // plan on the host and going up, the flat columns' emit kernel, the items going up
        float ms[6] = {};
        (void)hipEventSynchronize(ev[7]);
        const int pairs[6][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}};
        for (int k = 0; k < 6; ++k) (void)hipEventElapsedTime(&ms[k], ev[pairs[k][0]], ev[pairs[k][1]]);
        fprintf(stderr, "PQL_STEPS {\"rows_alloc_ms\": %.3f, \"count_scan_ms\": %.3f, \"totals_wait_ms\": %.3f, \"words_alloc_ms\": %.3f, \"levels_ms\": %.3f, "
                        "\"rank_scan_ms\": %.3f, \"tiles_ms\": %.3f, \"plan_ms\": %.3f, \"emit_ms\": %.3f}\n",
                host_ms[0], ms[0], host_ms[1], host_ms[2], ms[1], ms[2], ms[3], ms[4], ms[5]);
    }
    return OXH_OK;
}

}  // namespace oxh
