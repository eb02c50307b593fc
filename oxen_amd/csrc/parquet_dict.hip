// oxen_amd/csrc/parquet_dict.hip -- the dictionary chunks of the Parquet writer (OXH_PARQUET_DICTIONARY of
// oxh_write_parquet_*; the format is stated in include/oxen_hash.h "Parquet", DESIGN.md §4 "Parquet"). A chunk -- one
// row group's INT64, DOUBLE or string column -- is a candidate; whether it gets a dictionary is decided on the host
// (parquet_host.hpp dict_chunk) from what the first three steps leave:
//   insert   pqd_insert_kernel, a lane per row and candidate column, grid-stride. Each chunk owns an open-addressing
//            table of `slots` words (a power of two, at least twice the chunk's rows or 2 * kDictMaxEntries). A word is a
//            ROW of the chunk's column: claimed by compare-and-swap, and from then on the smallest row that joined
//            (atomic min). A lane that meets a taken word compares its own value with that row's actual value -- the 8
//            bytes, or the length and then the bytes -- and joins or probes on: the hash only picks where to start.
//            Every row of a word holds the same value, so it does not matter which of them a reader sees. Equal
//            neighbours in a wave elect their first lane, which probes for all of them; a lane whose row is above the
//            word it joins skips the atomic (the minimum cannot change). In front of the chunk's table a workgroup
//            keeps kPqdLdsSlots words in LDS (kPqdLdsLevel; group_count_kernel's pattern): 24 bits of the value's
//            hash above the smallest row of the chunk, in this workgroup, that joined, and beside it the word's
//            place in the chunk's table once the lane that claimed it knows it. A head lane whose tag matches
//            compares the actual values, as everywhere, and takes the place from LDS: a column of a hundred labels
//            costs LDS probes and cached loads, and one atomic min per word and workgroup when the workgroup leaves
//            the chunk. A tag that does not match costs no load, so a column of distinct values pays kPqdLdsProbes
//            LDS reads a row. Which row wins a swap differs from run to run; the word's final value, the value's
//            first row, does not. A counter of claimed words sets the chunk's overflow word past kDictMaxEntries, a string cell
//            above kDictMaxCell sets it too, and the lanes of such a chunk stop inserting. Every row records its
//            word's place (u32);
//   rank     pqd_flag_kernel marks the rows that are their word's row -- the first occurrences -- and the device-wide
//            exclusive_scan_u32 over the flags gives every first row its place among them; a chunk's base is the
//            place of its first row's element, so one scan serves all chunks. Strings: a second scan over 4 + length
//            of the flagged rows gives every entry's byte in its dictionary page. pqd_chunk_kernel leaves per chunk
//            the entries, the dictionary's bytes and the overflow word; they come down with the tile table;
//   index    pqd_index_kernel, after the plan has come up and beside the emit kernel's heads and levels: a wave per
//            (tile, candidate column) of a dictionary chunk. A first row gathers its entry to its place in the
//            dictionary page (an 8-byte store; a string's length word and bytes by its lane); every valid row's index
//            rank[first row of its word] - the chunk's base goes as a u32 to the page's span of a dense array, at the
//            row's rank in the page: the plan's tile base, the popcounts of the steps in front, mbcnt in the ballot;
//   pack     pqd_pack_kernel: a wave takes 512 indices of one page (64 groups of 8; a page's span starts at a multiple
//            of 512, so a block never straddles pages), every lane packs its group to `width` bytes, LSB first, into
//            the wave's LDS, and the 64 * width bytes leave as aligned 16-byte blocks on the destination's grid. Indices
//            behind the page's last valid row are 0 without being read: the pad.
// Every byte has one writer, every store is checked against the plan's sizes first, and what is inconsistent (columns
// that change during the call) sets the error word. No workgroup waits for another; launches order the steps.
#include "parquet_device.hpp"

using namespace oxh::capi;
namespace pq = oxh::parquet;

namespace oxh {

constexpr unsigned long long kPqdEmpty = ~0ull;  // no row is 2^64 - 1
constexpr uint32_t kPqdNone = 0xFFFFFFFFu;

// The insert's first level in LDS, kept on what tools/parquet_dict_probe.py measured (DESIGN.md §4 "Parquet"); the
// probe builds the other arm, and the arm that times the steps by events, by defining these.
#ifndef OXH_PQD_LDS_LEVEL
#define OXH_PQD_LDS_LEVEL 1
#endif
#ifndef OXH_PQD_STEP_EVENTS
#define OXH_PQD_STEP_EVENTS 0
#endif
constexpr bool kPqdLdsLevel = OXH_PQD_LDS_LEVEL;
// Open addressing, kPqdLdsProbes places a value; no new value is taken once three quarters are in use.
constexpr uint32_t kPqdLdsSlots = 512, kPqdLdsProbes = 4;
constexpr unsigned long long kPqdLdsRow = (1ull << 40) - 1;  // an LDS word: the hash's tag << 40 | row - the chunk's first row

struct PqdArgs {
    PqArgs a;
    const uint32_t* cand;        // candidate k: its column, then (at ncand + k) its ordinal among the string candidates
    uint32_t ncand, nstr, slots;
    uint64_t group_rows, ngroups;
    unsigned long long* tables;  // chunk (group * ncand + k): slots words
    unsigned long long* count;   // chunk: the claimed words, then the overflow word
    uint32_t* slot_of;           // k * nrows + row
    uint32_t* flag;              // ncand * nrows + 1: the dense array's memory, which nothing else uses before the plan
    uint64_t* place;             // as many: the scanned flags
    uint32_t* strlen_flag;       // string candidates: nstr * nrows + 1, then their scan
    uint64_t* strplace;
    uint32_t* dense;
    uint64_t dense_room;
};

__device__ __forceinline__ bool pqd_is_string(uint32_t type) { return type == OXH_CSV_STRING || type == OXH_CSV_STRING64; }

__device__ __forceinline__ uint64_t pqd_mix(uint64_t x) {
    x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27, x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t pqd_hash_bytes(const uint8_t* p, uint32_t n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
    uint32_t b = 0;
    for (; b + 8 <= n; b += 8) h = pqd_mix(h ^ ld64u(p + b));
    uint64_t last = 0;
    for (uint32_t k = 0; b + k < n; ++k) last |= (uint64_t)p[b + k] << (8 * k);
    return pqd_mix(h ^ last);
}
__device__ __forceinline__ bool pqd_equal_bytes(const uint8_t* p, const uint8_t* q, uint32_t n) {
    uint32_t b = 0;
    for (; b + 8 <= n; b += 8)
        if (ld64u(p + b) != ld64u(q + b)) return false;
    for (; b < n; ++b)
        if (p[b] != q[b]) return false;
    return true;
}

// ---------------------------------------------------------------- insert
// Row `rep` of the column holds this lane's value (its 8 bytes `word`; a string's `cell` bytes at `start`).
__device__ __forceinline__ bool pqd_same_value(const RowCol& c, bool str, uint64_t rep, uint64_t word, uint64_t start, uint64_t cell, unsigned long long& bad) {
    if (!str) return ld64u(c.values + 8 * rep) == word;
    uint64_t rep_start = 0;
    const uint64_t rep_cell = row_cell(c, rep, rep_start, bad);
    return rep_cell == cell && pqd_equal_bytes(c.values + start, c.values + rep_start, (uint32_t)cell);
}

// The workgroup leaves a chunk: every LDS word whose place in the chunk's table is known lowers that word to the
// smallest row that joined it here, and the table in LDS is empty again. Every lane of the workgroup calls it.
__device__ __forceinline__ void pqd_lds_flush(unsigned long long* lds_word, uint32_t* lds_slot, uint32_t& lds_used, unsigned long long* tab, uint32_t slots,
                                              uint64_t row0) {
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kPqdLdsSlots; s += 256) {
        const unsigned long long word = lds_word[s];
        const uint32_t slot = lds_slot[s];
        if (tab && word != kPqdEmpty && slot < slots) {  // a slot here is one this workgroup probed to in this table
            const unsigned long long r = row0 + (word & kPqdLdsRow);
            if (r < __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&tab[slot], r);
        }
        lds_word[s] = kPqdEmpty, lds_slot[s] = kPqdNone;
    }
    if (threadIdx.x == 0) lds_used = 0;
    __syncthreads();
}

__global__ __launch_bounds__(256) void pqd_insert_kernel(const PqdArgs d, unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long lds_word[kPqdLdsLevel ? kPqdLdsSlots : 1];
    __shared__ uint32_t lds_slot[kPqdLdsLevel ? kPqdLdsSlots : 1], lds_used;
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = d.a.nrows, stride = (uint64_t)gridDim.x * 256, rounds = (n + stride - 1) / stride;
    const bool lds = kPqdLdsLevel && d.group_rows <= kPqdLdsRow;  // a row of the chunk fits an LDS word
    unsigned long long bad = 0;
    unsigned long long* lds_tab = nullptr;  // the chunk whose values the LDS words hold: uniform in the workgroup
    uint64_t lds_row0 = 0;
    if (lds) pqd_lds_flush(lds_word, lds_slot, lds_used, nullptr, 0, 0);
    for (uint32_t k = blockIdx.y; k < d.ncand; k += gridDim.y) {
        const PqCol& pc = d.a.cols[d.cand[k]];
        const bool str = pqd_is_string(pc.type);
        for (uint64_t t = 0; t < rounds; ++t) {  // uniform: every lane reaches the shuffles and the barriers
            // a workgroup's 256 rows start at a multiple of 256: one tile, so one chunk
            const uint64_t r_wg = t * stride + (uint64_t)blockIdx.x * 256, r = r_wg + threadIdx.x;
            if (lds && r_wg < n) {
                unsigned long long* const now = d.tables + ((r_wg / d.group_rows) * d.ncand + k) * d.slots;
                if (now != lds_tab) {
                    pqd_lds_flush(lds_word, lds_slot, lds_used, lds_tab, d.slots, lds_row0);
                    lds_tab = now, lds_row0 = r_wg / d.group_rows * d.group_rows;
                }
            }
            bool live = r < n && pqw_present(pc.c, r);
            const uint64_t chunk = live ? (r / d.group_rows) * d.ncand + k : 0;
            unsigned long long* const tab = d.tables + chunk * d.slots;
            unsigned long long* const over = d.count + 2 * chunk + 1;
            uint64_t start = 0, cell = 8, word = 0;  // the 8 bytes; strings: their hash
            if (live && !str) word = ld64u(pc.c.values + 8 * r);
            if (live && str) {
                cell = row_cell(pc.c, r, start, bad);
                if (cell > pq::kDictMaxCell) {
                    __hip_atomic_store(over, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    live = false;
                } else {
                    word = pqd_hash_bytes(pc.c.values + start, (uint32_t)cell);
                }
            }
            if (live && __hip_atomic_load(over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) live = false;  // the chunk stays PLAIN
            // equal neighbours elect their first lane
            const uint64_t word_up = (uint64_t)__shfl_up((long long)word, 1, 64), cell_up = (uint64_t)__shfl_up((long long)cell, 1, 64);
            const uint64_t start_up = (uint64_t)__shfl_up((long long)start, 1, 64);
            const bool live_up = __shfl_up((int)live, 1, 64) != 0;
            bool same = lane > 0 && live && live_up && word_up == word && cell_up == cell;
            if (same && str) same = pqd_equal_bytes(pc.c.values + start, pc.c.values + start_up, (uint32_t)cell);
            const bool head = live && !same;
            const unsigned long long heads = __ballot(head);
            uint32_t slot = kPqdNone, mine = kPqdNone;  // mine: the LDS word this lane claimed, whose place it owes
            const uint64_t mixed = head ? pqd_mix(word) : 0;
            if (lds && head) {
                const unsigned long long tag = (mixed >> 40) << 40, rel = r - lds_row0;
                uint32_t s = (uint32_t)(mixed >> 31) & (kPqdLdsSlots - 1);
                for (uint32_t p = 0; p < kPqdLdsProbes; ++p, s = (s + 1) & (kPqdLdsSlots - 1)) {
                    unsigned long long have = __hip_atomic_load(&lds_word[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (have == kPqdEmpty) {
                        if (__hip_atomic_load(&lds_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= kPqdLdsSlots / 4 * 3) break;
                        have = atomicCAS(&lds_word[s], kPqdEmpty, tag | rel);  // a word never is empty again before the flush
                        if (have == kPqdEmpty) {
                            atomicAdd(&lds_used, 1u);
                            mine = s;
                            break;
                        }
                    }
                    if ((have >> 40) << 40 != tag) continue;
                    const uint64_t rep = lds_row0 + (have & kPqdLdsRow);  // a row this workgroup has read: the actual values decide
                    if (!pqd_same_value(pc.c, str, rep, word, start, cell, bad)) continue;
                    slot = __hip_atomic_load(&lds_slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (slot != kPqdNone && rel < (have & kPqdLdsRow)) atomicMin(&lds_word[s], tag | rel);  // the flush takes it to the table
                    break;  // a place not yet known: this lane finds it in the chunk's table itself
                }
            }
            if (head && slot == kPqdNone) {
                const uint32_t mask = d.slots - 1;
                uint32_t s = (uint32_t)mixed & mask;
                for (uint32_t p = 0; p < d.slots; ++p, s = (s + 1) & mask) {
                    unsigned long long rep = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (rep == kPqdEmpty) {
                        if (__hip_atomic_load(over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                        rep = atomicCAS(&tab[s], kPqdEmpty, (unsigned long long)r);  // a word never is empty again
                        if (rep == kPqdEmpty) {
                            const unsigned long long claimed = __hip_atomic_fetch_add(d.count + 2 * chunk, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
                            if (claimed > pq::kDictMaxEntries) __hip_atomic_store(over, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            slot = s;
                            break;
                        }
                    }
                    if (rep >= n) {  // not a row: never read through it
                        bad |= kPqErrPlace;
                        break;
                    }
                    if (pqd_same_value(pc.c, str, rep, word, start, cell, bad)) {
                        if (r < rep) atomicMin(&tab[s], (unsigned long long)r);  // a row above the word's cannot change it
                        slot = s;
                        break;
                    }
                }
            }
            if (mine != kPqdNone && slot != kPqdNone) __hip_atomic_store(&lds_slot[mine], slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long upto = lane == 63 ? heads : heads & ((2ull << lane) - 1);
            const int head_lane = upto ? 63 - __builtin_clzll(upto) : 0;
            slot = (uint32_t)__shfl((int)slot, head_lane, 64);
            if (live) d.slot_of[(uint64_t)k * n + r] = slot;
        }
    }
    if (lds) pqd_lds_flush(lds_word, lds_slot, lds_used, lds_tab, d.slots, lds_row0);
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- rank
// flag[k * nrows + r] = row r is the first occurrence of its value in its chunk (0 in a chunk that overflowed);
// strings: strlen_flag = 4 + length of those rows. The element behind the last row is 0: its scan is the total.
__global__ __launch_bounds__(256) void pqd_flag_kernel(const PqdArgs d, unsigned long long* __restrict__ ctrl) {
    const uint64_t n = d.a.nrows, stride = (uint64_t)gridDim.x * 256;
    unsigned long long bad = 0;
    for (uint32_t k = blockIdx.y; k < d.ncand; k += gridDim.y) {
        const PqCol& pc = d.a.cols[d.cand[k]];
        const uint32_t ks = d.cand[d.ncand + k];
        for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
            const uint64_t chunk = (r / d.group_rows) * d.ncand + k;
            bool first = false;
            if (pqw_present(pc.c, r) && !d.count[2 * chunk + 1]) {
                const uint32_t slot = d.slot_of[(uint64_t)k * n + r];
                if (slot < d.slots)
                    first = d.tables[chunk * d.slots + slot] == r;
                else
                    bad |= kPqErrPlace;  // a chunk that did not overflow placed every row
            }
            d.flag[(uint64_t)k * n + r] = first;
            if (ks != kPqdNone) {
                uint64_t start = 0;
                const uint64_t cell = first ? row_cell(pc.c, r, start, bad) : 0;
                d.strlen_flag[(uint64_t)ks * n + r] = first && cell <= pq::kDictMaxCell ? 4 + (uint32_t)cell : 0;
            }
        }
        if (k == d.ncand - 1 && blockIdx.x == 0 && threadIdx.x == 0) {
            d.flag[(uint64_t)d.ncand * n] = 0;
            d.strlen_flag[(uint64_t)d.nstr * n] = 0;
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A lane per (row group, candidate): what the planner reads, at group * ncols + column.
__global__ __launch_bounds__(256) void pqd_chunk_kernel(const PqdArgs d, pq::ChunkDict* __restrict__ chunks) {
    const uint64_t n = d.a.nrows, items = d.ngroups * d.ncand;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256) {
        const uint64_t g = i / d.ncand, r0 = g * d.group_rows, r1 = r0 + d.group_rows < n ? r0 + d.group_rows : n;
        const uint32_t k = (uint32_t)(i % d.ncand), ks = d.cand[d.ncand + k];
        pq::ChunkDict c;
        c.num_values = d.place[(uint64_t)k * n + r1] - d.place[(uint64_t)k * n + r0];
        c.dict_bytes = ks == kPqdNone ? 8 * c.num_values : d.strplace[(uint64_t)ks * n + r1] - d.strplace[(uint64_t)ks * n + r0];
        c.overflow = d.count[2 * i + 1];
        chunks[g * d.a.ncols + d.cand[k]] = c;
    }
}

// ---------------------------------------------------------------- the dictionary pages' entries, the dense indices
__global__ __launch_bounds__(256) void pqd_index_kernel(const PqdArgs d, const PqEmit e, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = d.a.nrows, items = d.a.ntiles * d.ncand, nwaves = (uint64_t)gridDim.x * 4;
    unsigned long long bad = 0;
    for (uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += nwaves) {  // uniform in the wave
        const uint32_t k = (uint32_t)(item % d.ncand), col = d.cand[k], ks = d.cand[d.ncand + k];
        const PqCol& pc = d.a.cols[col];
        const uint64_t tile = item / d.ncand, r0 = tile * pq::kTileRows;
        const pq::Place pl = e.places[tile * d.a.ncols + col];
        if (pl.page >= e.npages) {
            bad |= kPqErrPlace;
            continue;
        }
        const pq::Page pg = e.pages[pl.page];
        if (!pg.dict_width) continue;  // a PLAIN chunk: the emit kernel's
        if (pg.dict_page >= e.npages || tile < pg.tile0 || r0 < pg.row0 || r0 >= pg.row0 + pg.rows || pl.rank_base > pg.nvalid) {
            bad |= kPqErrPlace;
            continue;
        }
        const pq::Page dp = e.pages[pg.dict_page];
        uint8_t* const body = e.out + dp.file_at + dp.head_len;
        const uint64_t g = r0 / d.group_rows, flat0 = (uint64_t)k * n + g * d.group_rows;
        unsigned long long* const tab = d.tables + (g * d.ncand + k) * d.slots;
        const uint64_t place0 = d.place[flat0], byte0 = ks == kPqdNone ? 0 : d.strplace[(uint64_t)ks * n + g * d.group_rows];
        const uint32_t steps = n - r0 < pq::kTileRows ? (uint32_t)((n - r0 + 63) / 64) : 16u;
        uint32_t cnt = 0;
        for (uint32_t s = 0; s < steps; ++s) {
            const uint64_t r = r0 + 64 * s + lane;
            const bool live = r < n && pqw_present(pc.c, r);
            const unsigned long long mask = __ballot(live);
            const uint32_t rank = pl.rank_base + cnt + pqw_below(mask);
            cnt += (uint32_t)__popcll(mask);
            if (!live) continue;
            const uint32_t slot = d.slot_of[(uint64_t)k * n + r];
            const uint64_t first = slot < d.slots ? tab[slot] : kPqdEmpty;
            if (first > r || first < g * d.group_rows) {  // the first occurrence is a row of the chunk at or before this one
                bad |= kPqErrPlace;
                continue;
            }
            const uint64_t entry = d.place[(uint64_t)k * n + first] - place0;
            if (entry >= dp.nvalid || rank >= pg.nvalid || pg.dense_at + rank >= d.dense_room) {
                bad |= kPqErrPlace;
                continue;
            }
            d.dense[pg.dense_at + rank] = (uint32_t)entry;
            if (first != r) continue;
            if (ks == kPqdNone) {
                const uint64_t v = ld64u(pc.c.values + 8 * r);
                if (8 * (entry + 1) <= dp.values_bytes)
                    __builtin_memcpy(body + 8 * entry, &v, 8);
                else
                    bad |= kPqErrPlace;
            } else {
                uint64_t start = 0;
                const uint64_t cell = row_cell(pc.c, r, start, bad), at = d.strplace[(uint64_t)ks * n + r] - byte0;
                if (cell <= pq::kDictMaxCell && at <= dp.values_bytes && at + 4 + cell <= dp.values_bytes) {
                    const uint32_t len = (uint32_t)cell;
                    __builtin_memcpy(body + at, &len, 4);
                    copy_span_lane(body + at + 4, pc.c.values + start, len);
                } else {
                    bad |= kPqErrPlace;
                }
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- pack
constexpr uint32_t kPqdStage = 64 * 16 + 32;  // 64 groups at the widest index, at the destination's misalignment

__global__ __launch_bounds__(256) void pqd_pack_kernel(const PqdArgs d, const PqEmit e, const PqdPack* __restrict__ packs, uint64_t npacks,
                                                       uint64_t nblocks, unsigned long long* __restrict__ ctrl) {
    __shared__ __attribute__((aligned(16))) uint8_t stages[4][kPqdStage];
    const unsigned lane = threadIdx.x & 63;
    uint8_t* const stage = stages[threadIdx.x >> 6];
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    unsigned long long bad = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblocks; b += nwaves) {  // uniform in the wave
        const uint64_t x = b * pq::kDenseBlock;
        uint64_t lo = 0, hi = npacks;  // the last page whose span starts at or before x
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (packs[mid].dense_at <= x) lo = mid; else hi = mid;
        }
        if (packs[lo].page >= e.npages) {
            bad |= kPqErrPlace;
            continue;
        }
        const pq::Page pg = e.pages[packs[lo].page];
        const uint32_t w = pg.dict_width;
        if (w == 0 || w > 16 || pg.dense_at != packs[lo].dense_at || x < pg.dense_at) {
            bad |= kPqErrPlace;
            continue;
        }
        const uint64_t k0 = x - pg.dense_at, groups = ((uint64_t)pg.nvalid + 7) / 8, g0 = k0 / 8;
        if (g0 >= groups) continue;  // behind the page's last group
        const uint32_t ng = groups - g0 < 64 ? (uint32_t)(groups - g0) : 64u;
        const uint64_t prefix = 1 + pq::varint_len((groups << 1) | 1);
        if (prefix + (g0 + ng) * w > pg.values_bytes || x + 8ull * ng > d.dense_room) {  // never a store outside the page's values
            bad |= kPqErrPlace;
            continue;
        }
        uint8_t* const dst = e.out + pg.file_at + pg.head_len + pg.level_bytes + prefix + g0 * w;
        const uint32_t shift = (uint32_t)((uintptr_t)dst & 15);
        if (lane < ng) {
            uint64_t acc_lo = 0, acc_hi = 0;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint64_t at = k0 + 8 * lane + j;
                const uint64_t idx = at < pg.nvalid ? d.dense[pg.dense_at + at] : 0;  // the pad is 0
                if (idx >> w) bad |= kPqErrPlace;
                const uint32_t bit = j * w;  // < 128
                if (bit < 64) {
                    acc_lo |= idx << bit;
                    if (bit + w > 64) acc_hi |= idx >> (64 - bit);
                } else {
                    acc_hi |= idx << (bit - 64);
                }
            }
            uint8_t* const p = stage + shift + lane * w;
            for (uint32_t t = 0; t < w; ++t) p[t] = (uint8_t)(t < 8 ? acc_lo >> (8 * t) : acc_hi >> (8 * (t - 8)));
        }
        pqw_wave_lds_order();  // the block is assembled
        pqw_store_span(dst, (uint64_t)ng * w, stage, lane);
        pqw_wave_lds_order();  // and stored: the next one may overwrite it
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- the call's side
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~255ull; }
unsigned rows_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 2048); }

// OXH_PQD_STEP_EVENTS (a probe's library, one call at a time): events around the steps of a call; write() waits for
// the last and leaves one line on stderr. The shipped library records nothing.
#if OXH_PQD_STEP_EVENTS
hipEvent_t g_step[6];
void step_mark(int k, hipStream_t st) {
    if (!g_step[k]) (void)hipEventCreate(&g_step[k]);
    (void)hipEventRecord(g_step[k], st);
}
void step_report(bool wrote) {
    float ms[4] = {0, 0, 0, 0};
    (void)hipEventSynchronize(g_step[wrote ? 5 : 2]);
    for (int k = 0; k < (wrote ? 4 : 2); ++k) (void)hipEventElapsedTime(&ms[k], g_step[k + (k > 1)], g_step[k + (k > 1) + 1]);
    fprintf(stderr, "PQD_STEPS {\"insert_ms\": %.3f, \"rank_ms\": %.3f, \"gather_ms\": %.3f, \"pack_ms\": %.3f}\n", ms[0], ms[1], ms[2], ms[3]);
}
#else
inline void step_mark(int, hipStream_t) {}
inline void step_report(bool) {}
#endif
}  // namespace

void PqDict::layout(uint64_t nrows, uint32_t ncols, const uint32_t* types, uint64_t rows_per_group) {
    group_rows = rows_per_group, ngroups = (nrows + group_rows - 1) / group_rows;
    ncand = nstr = 0;
    for (uint32_t c = 0; c < ncols; ++c)
        if (pq::dict_candidate(types[c])) ++ncand, nstr += pq::is_string(types[c]);
    const uint64_t chunk_rows = std::min(group_rows, nrows), ntiles = (nrows + pq::kTileRows - 1) / pq::kTileRows;
    slots = 64;
    while (slots < 2 * pq::kDictMaxEntries && slots < 2 * chunk_rows) slots *= 2;
    nflat = (uint64_t)ncand * nrows, nflat_str = (uint64_t)nstr * nrows;
    const uint64_t dense_room = nflat + pq::kDenseBlock * std::max<uint64_t>(ntiles, 1) * ncand;  // every page pads its span to a block, and holds a tile; the flags' nflat + 1
    at_cand = 0;
    at_tables = up256(at_cand + 2ull * ncand * 4);
    at_count = at_tables + ngroups * ncand * slots * 8;
    at_slot = up256(at_count + ngroups * ncand * 16);
    at_dense = up256(at_slot + nflat * 4);
    at_place = up256(at_dense + dense_room * 4);
    at_sums = at_place + (nflat + 1) * 8;
    at_strlen = up256(at_sums + (scan_tiles(nflat + 1) + 1) * 8);
    at_strplace = up256(at_strlen + (nflat_str + 1) * 4);
    at_strsums = at_strplace + (nflat_str + 1) * 8;
    at_packs = up256(at_strsums + (scan_tiles(nflat_str + 1) + 1) * 8);
    total = up256(at_packs + ntiles * ncand * sizeof(PqdPack));
}

uint64_t PqDict::work_bytes(uint64_t nrows, uint32_t ncols, const uint32_t* types, uint64_t group_rows) {
    PqDict d;
    d.layout(nrows, ncols, types, group_rows);
    return d.ncand ? d.total : 0;
}

namespace {
PqdArgs device_args(const PqDict& d, const PqArgs& args) {
    PqdArgs x{};
    uint8_t* w = d.d_work;
    x.a = args, x.cand = (const uint32_t*)(w + d.at_cand), x.ncand = d.ncand, x.nstr = d.nstr, x.slots = d.slots;
    x.group_rows = d.group_rows, x.ngroups = d.ngroups;
    x.tables = (unsigned long long*)(w + d.at_tables), x.count = (unsigned long long*)(w + d.at_count);
    x.slot_of = (uint32_t*)(w + d.at_slot), x.dense = (uint32_t*)(w + d.at_dense), x.place = (uint64_t*)(w + d.at_place);
    x.strlen_flag = (uint32_t*)(w + d.at_strlen), x.strplace = (uint64_t*)(w + d.at_strplace);
    x.flag = x.dense;
    x.dense_room = (d.at_place - d.at_dense) / 4;
    return x;
}
}  // namespace

int PqDict::build(const PqArgs& args, const uint32_t* types, uint64_t rows_per_group, uint8_t* work, pq::ChunkDict* d_chunks,
                  unsigned long long* d_ctrl, hipStream_t st) {
    layout(args.nrows, args.ncols, types, rows_per_group);
    d_work = work;
    if (!ncand) return OXH_OK;
    cand.assign(2 * (size_t)ncand, kPqdNone);
    for (uint32_t c = 0, k = 0, ks = 0; c < args.ncols; ++c) {
        if (!pq::dict_candidate(types[c])) continue;
        cand[k] = c;
        if (pq::is_string(types[c])) cand[ncand + k] = ks++;
        ++k;
    }
    const PqdArgs x = device_args(*this, args);
    HIP_TRY(hipMemcpyAsync(d_work + at_cand, cand.data(), cand.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(x.tables, 0xFF, ngroups * ncand * slots * 8, st));
    HIP_TRY(hipMemsetAsync(x.count, 0, ngroups * ncand * 16, st));
    const dim3 grid(rows_grid(args.nrows), std::min<uint32_t>(ncand, 65535));
    step_mark(0, st);
    pqd_insert_kernel<<<grid, 256, 0, st>>>(x, d_ctrl);
    HIP_TRY(hipGetLastError());
    step_mark(1, st);
    pqd_flag_kernel<<<grid, 256, 0, st>>>(x, d_ctrl);
    HIP_TRY(hipGetLastError());
    int rc = exclusive_scan_u32(x.flag, nflat + 1, x.place, (unsigned long long*)(d_work + at_sums), st);
    if (rc) return rc;
    if ((rc = exclusive_scan_u32(x.strlen_flag, nflat_str + 1, x.strplace, (unsigned long long*)(d_work + at_strsums), st))) return rc;
    pqd_chunk_kernel<<<(unsigned)std::min<uint64_t>((ngroups * ncand + 255) / 256, 1024), 256, 0, st>>>(x, d_chunks);
    HIP_TRY(hipGetLastError());
    step_mark(2, st);
    return OXH_OK;
}

int PqDict::write(const PqArgs& args, const PqEmit& em, const pq::Plan& plan, unsigned long long* d_ctrl, hipStream_t st) {
    if (!plan.dense_indices) {  // no chunk has a dictionary
        step_report(false);
        return OXH_OK;
    }
    const PqdArgs x = device_args(*this, args);
    packs.clear();
    for (size_t k = 0; k < plan.pages.size(); ++k)
        if (plan.pages[k].dict_width && plan.pages[k].rows) packs.push_back(PqdPack{plan.pages[k].dense_at, (uint32_t)k, 0});
    if (plan.dense_indices > x.dense_room || plan.pages.size() > kPqdNone || packs.size() > args.ntiles * ncand)
        return fail(OXH_ERR_HIP, "parquet write: the dictionary indices outgrew their room");
    HIP_TRY(hipMemcpyAsync(d_work + at_packs, packs.data(), packs.size() * sizeof(PqdPack), hipMemcpyHostToDevice, st));
    step_mark(3, st);
    pqd_index_kernel<<<(unsigned)std::min<uint64_t>((args.ntiles * ncand + 3) / 4, kPqMaxGroups), 256, 0, st>>>(x, em, d_ctrl);
    HIP_TRY(hipGetLastError());
    step_mark(4, st);
    const uint64_t nblocks = plan.dense_indices / pq::kDenseBlock;
    pqd_pack_kernel<<<(unsigned)std::min<uint64_t>((nblocks + 3) / 4, kPqMaxGroups), 256, 0, st>>>(x, em, (const PqdPack*)(d_work + at_packs), packs.size(),
                                                                                                  nblocks, d_ctrl);
    HIP_TRY(hipGetLastError());
    step_mark(5, st);
    step_report(true);
    return OXH_OK;
}

}  // namespace oxh
