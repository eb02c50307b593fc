// oxen_amd/csrc/parquet_lists.hip -- the list columns of a Parquet handle (oxh_parquet_lists_*): the repetition and
// definition levels of a three-level LIST of INT32 / INT64 / FLOAT / DOUBLE to Arrow's offsets, the lists' validity,
// the elements' validity and the element values. The format, the refusals and the limits are stated in
// include/oxen_hash.h "Parquet: the file's bytes"; the schema's lists and the page lists are parquet_read_host.hpp's
// (Leaf, ListPage, list_pages), the handle and the value of a rank parquet_read_device.hpp's, the run chase and the
// bit extraction parquet_bits.hpp's.
//
// A page's level entries are not its rows: a row is the entries from one of repetition level 0 up to the next, it may
// have no element (a null or an empty list: one entry below def_slot) and it may run on through the following
// pages. So row -> entry and element -> value are rank / select problems over three bit vectors. Per selected column,
// on one stream (launches order the steps, no workgroup waits for another):
//   levels    pql_levels_kernel, a wave per data page: both hybrid streams are chased together by the whole wave
//             (uniform control flow, every lane reads the same run header; an RLE run costs no load), 64 entries a
//             round, lane j holding entry j's two levels in registers. Four ballots a round -- start (rep == 0), slot
//             (def >= def_slot: an element, null or not), value (def == max_def) and, for a start, valid (def >=
//             def_list: the list is not null) -- leave as words with the page's starts, slots and values in front of
//             them, then the page's three totals. A V1 page's definition stream is found here (its length follows the
//             repetition stream), and the page's record for the index pass and the gather is written. A malformed
//             stream, a level above max_def or a chunk that does not begin with a row sets the error word; the
//             words it did not reach are zeros;
//   bases     exclusive_scan_u32 over the pages' starts and over their slots: page p's first row start is row
//             row0[p], its first slot element slot0[p] (64-bit). The totals come down: the starts of every row group's
//             pages must be its rows, the slots are the element count the caller's buffers are checked against;
//   indices   pq_index_kernel (parquet_read.hip) over the records the level pass wrote, for dictionary-coded pages;
//   rows      pql_rows_kernel, a lane per output row: its page by a search of row0, its word by a search of the
//             start-prefixes, its entry by selecting the n-th set bit of `start`; offsets[row] = slot0 + the slots in
//             front of that entry, as int32 or int64; the lists' validity leaves as ballots, 8 bytes a wave;
//   elements  pql_elements_kernel, a lane per output element: page, word and entry the same way over the slots; the
//             value bit and the value's rank in its page; the value from the PLAIN body at rank * width (any
//             alignment) or from dict[index[rank]], widened in the store, stored coalesced at values[slot]; a null
//             element is 0; the elements' validity leaves as ballots.
// One writer per output byte; no result depends on what scratch or the outputs held; every load is bounded by the
// page or run it belongs to, and a rank the words do not hold (a buffer that changed under the call) stores 0 and
// sets the error word. Slots per call: 64-bit. Not measured against a lane per entry that scatters to its slot.
#include "parquet_read_device.hpp"

using namespace oxh::capi;

namespace oxh {

namespace pql {
constexpr int kColNullLists = pqr::kColNulls, kColNullElements = pqr::kColBytes;  // beside kColDictValues, kColErr
}

// What the list kernels read of one column.
struct PqList {
    PqColumn c;  // bytes, image, dicts, idx as ever; pages: the records the level pass writes; page_valid: a page's values
    const pqr::ListPage* lp;
    pqr::DataPage* records;
    uint32_t def_list, def_slot, max_def, width;
    uint64_t *start_w, *slot_w, *value_w, *valid_w;  // per 64 level entries of a page
    uint32_t *pre_start, *pre_slot, *pre_value;      // per word: the page's starts, slots and values in front of it
    uint32_t *page_starts, *page_slots;              // per page
    const uint64_t *row0, *slot0;                    // their exclusive sums
    uint64_t nslots;
};

// One hybrid stream as the wave walks it: the run it stands in and what is left of it.
struct PqlStream {
    pqr::Span s;
    pqr::Run r;
    uint64_t left, at;
    uint32_t w;
    bool ok;
};

// The levels of the stream's next len <= 64 entries, lane j's returned to lane j; `missing`: the entries the page
// still lacks. Uniform in the wave.
__device__ __forceinline__ uint32_t pql_take(PqlStream& t, uint64_t missing, uint32_t len, unsigned lane) {
    uint32_t mine = 0, filled = 0;
    while (filled < len) {
        if (t.left == 0) {
            if (!pqr::next_run(t.s, t.w, missing - filled, t.r)) {
                t.ok = false;
                break;
            }
            t.left = t.r.count, t.at = 0;
        }
        const uint32_t take = (uint32_t)(t.left < len - filled ? t.left : len - filled);
        if (lane >= filled && lane < filled + take) mine = t.r.packed ? pqr::extract(t.r.body, t.r.avail, t.at + (lane - filled), t.w) : t.r.value;
        t.left -= take, t.at += take, filled += take;
    }
    return mine;
}

__global__ __launch_bounds__(256) void pql_levels_kernel(const PqList L, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long null_lists = 0, null_elements = 0, bad = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < L.c.npages; p += (uint64_t)gridDim.x * 4) {  // uniform in the wave
        const pqr::ListPage pg = L.lp[p];
        const uint8_t* body = pq_body(L.c, pg);
        const uint64_t n = pg.num_values, nwords = (n + 63) / 64;
        uint32_t def_at = pg.def_at, def_bytes = pg.def_bytes, values_at = pg.values_at;
        bool ok = true;
        if (def_at == ~0u) {  // V1: the definition stream's length follows the repetition stream
            const uint64_t room = pg.body_size - values_at;  // the page list holds values_at <= body_size
            def_bytes = room >= 4 ? pqr::le32(body + values_at) : 0;
            if (room < 4 || def_bytes > room - 4) ok = false, def_bytes = 0, def_at = values_at = pg.body_size;
            else def_at = values_at + 4, values_at = def_at + def_bytes;
        }
        PqlStream rep{{body + pg.rep_at, pg.rep_bytes, 0, false}, {}, 0, 0, 1, true};
        PqlStream def{{body + def_at, def_bytes, 0, false}, {}, 0, 0, L.width, true};
        uint32_t starts = 0, slots = 0, values = 0;
        uint64_t w = 0;
        for (; w < nwords && ok; ++w) {
            const uint64_t missing = n - 64 * w;
            const uint32_t len = (uint32_t)(missing < 64 ? missing : 64);
            const uint32_t r = pql_take(rep, missing, len, lane), d = pql_take(def, missing, len, lane);
            const bool in = lane < len;
            if (!rep.ok || !def.ok || __ballot(in && d > L.max_def)) {
                ok = false;
                break;
            }
            const uint64_t start = __ballot(in && r == 0), slot = __ballot(in && d >= L.def_slot), value = __ballot(in && d == L.max_def);
            const uint64_t valid = __ballot(in && r == 0 && d >= L.def_list);
            if (w == 0 && pg.first && !(start & 1)) bad |= pqr::kErrLevels;  // a chunk begins with a row
            if (lane == 0) {
                const uint64_t at = pg.word0 + w;
                L.start_w[at] = start, L.slot_w[at] = slot, L.value_w[at] = value, L.valid_w[at] = valid;
                L.pre_start[at] = starts, L.pre_slot[at] = slots, L.pre_value[at] = values;
            }
            starts += (uint32_t)__popcll(start), slots += (uint32_t)__popcll(slot), values += (uint32_t)__popcll(value);
            null_lists += (unsigned long long)__popcll(start & ~valid), null_elements += (unsigned long long)__popcll(slot & ~value);
        }
        for (uint64_t at = pg.word0 + w + lane; at < pg.word0 + nwords; at += 64) {  // what a malformed stream did not reach
            L.start_w[at] = L.slot_w[at] = L.value_w[at] = L.valid_w[at] = 0;
            L.pre_start[at] = starts, L.pre_slot[at] = slots, L.pre_value[at] = values;
        }
        if (lane == 0) {
            L.page_starts[p] = starts, L.page_slots[p] = slots, L.c.page_valid[p] = values;
            L.records[p] = pqr::DataPage{pg.word0 * 64, pg.word0, pg.body, pg.num_values, pg.body_size, def_at, def_bytes, values_at, pg.encoding, pg.dict, pg.in_image};
        }
        if (!ok) bad |= pqr::kErrLevels;
    }
    if (lane == 0) {
        if (null_lists) atomicAdd(&ctrl[pql::kColNullLists], null_lists);
        if (null_elements) atomicAdd(&ctrl[pql::kColNullElements], null_elements);
        if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The last k < n with a[k] <= x; a[0] <= x.
template <class T>
__device__ __forceinline__ uint32_t pql_last_le(const T* a, uint32_t n, T x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Where the n-th set bit of w is (n from 0, below popcount(w)): six halvings.
__device__ __forceinline__ uint32_t pql_select(uint64_t w, uint32_t n) {
    uint32_t at = 0;
#pragma unroll
    for (uint32_t half = 32; half; half >>= 1) {
        const uint32_t low = (uint32_t)__popcll(w & ((1ull << half) - 1));
        if (n >= low) n -= low, w >>= half, at += half;
    }
    return at;
}

// The entry that holds item `i` of the column's items -- row starts (base = row0, words = start_w) or element slots
// (slot0, slot_w): its page, its word and its bit. false: the words do not hold it.
__device__ __forceinline__ bool pql_locate(const PqList& L, const uint64_t* base, const uint32_t* page_items, const uint32_t* pre, const uint64_t* words,
                                           uint64_t i, uint32_t& page, uint64_t& word, uint32_t& bit) {
    page = pql_last_le(base, L.c.npages, i);
    const pqr::ListPage& pg = L.lp[page];
    const uint64_t local = i - base[page];
    word = pg.word0, bit = 0;
    if (local >= page_items[page]) return false;
    word += pql_last_le(pre + pg.word0, (pg.num_values + 63) / 64, (uint32_t)local);
    const uint32_t nth = (uint32_t)local - pre[word];
    if (nth >= (uint32_t)__popcll(words[word])) return false;
    bit = pql_select(words[word], nth);
    return true;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void pql_rows_kernel(const PqList L, void* __restrict__ offsets, uint8_t* __restrict__ validity,
                                                       unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = L.c.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballot
    bool bad = false;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool valid = false;
        if (i < n) {
            uint32_t page, bit;
            uint64_t word, at = 0;
            if (pql_locate(L, L.row0, L.page_starts, L.pre_start, L.start_w, i, page, word, bit)) {
                at = L.slot0[page] + L.pre_slot[word] + (uint64_t)__popcll(L.slot_w[word] & ((1ull << bit) - 1));
                valid = (L.valid_w[word] >> bit) & 1;
            } else {
                bad = true;
            }
            if (at > L.nslots) bad = true, at = L.nslots;
            if (WIDE) {
                ((uint64_t*)offsets)[i] = at;
                if (i + 1 == n) ((uint64_t*)offsets)[n] = L.nslots;
            } else {
                ((uint32_t*)offsets)[i] = (uint32_t)at;
                if (i + 1 == n) ((uint32_t*)offsets)[n] = (uint32_t)L.nslots;
            }
        }
        pq_store_word(validity, __ballot(valid), i - lane, n, lane);
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], pqr::kErrPlace, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// SRC: the bytes of a value in the file; DST: of a cell of `values` (pq_fixed_load).
template <uint32_t SRC, uint32_t DST, bool FLOAT>
__global__ __launch_bounds__(256) void pql_elements_kernel(const PqList L, void* __restrict__ values, uint8_t* __restrict__ child_validity,
                                                           unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = L.nslots, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballot
    bool lost = false, bad = false;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool valid = false;
        if (i < n) {
            uint32_t page, bit;
            uint64_t word, out = 0;
            if (pql_locate(L, L.slot0, L.page_slots, L.pre_slot, L.slot_w, i, page, word, bit)) {
                const uint64_t vw = L.value_w[word];
                valid = (vw >> bit) & 1;
                const uint32_t rank = L.pre_value[word] + (uint32_t)__popcll(vw & ((1ull << bit) - 1));
                if (valid && rank < L.c.page_valid[page]) {
                    const uint8_t* src = pq_fixed_source<SRC>(L.c, L.c.pages[page], rank, bad);
                    if (src) out = pq_fixed_load<SRC, DST, FLOAT>(src);
                } else if (valid) {
                    lost = true;
                }
            } else {
                lost = true;
            }
            if (DST == 8)
                ((uint64_t*)values)[i] = out;
            else
                ((uint32_t*)values)[i] = (uint32_t)out;
        }
        pq_store_word(child_validity, __ballot(valid), i - lane, n, lane);
    }
    if (bad || lost)
        __hip_atomic_fetch_or(&ctrl[pqr::kColErr], (bad ? pqr::kErrValues : 0) | (lost ? pqr::kErrPlace : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oxh

namespace {

namespace csv = oxh::csv;
namespace pqr = oxh::pqr;
using oxh::ParquetHandle;
using oxh::PqList;

// Working memory of one selected column (offsets into a lease); the columns run one after the other in it.
struct ListLease {
    uint64_t ctrl, lp, records, dicts, start_w, slot_w, value_w, valid_w, pre_start, pre_slot, pre_value, page_starts, page_slots, page_values, row0, slot0,
        idx, sums, total;
    ListLease(uint32_t nsel, uint64_t npages, uint64_t ndicts, uint64_t words) {
        csv::Carver carve;
        ctrl = carve((uint64_t)nsel * pqr::kColWords * 8);
        lp = carve(npages * sizeof(pqr::ListPage)), records = carve(npages * sizeof(pqr::DataPage)), dicts = carve(ndicts * sizeof(pqr::DictPage));
        start_w = carve(words * 8), slot_w = carve(words * 8), value_w = carve(words * 8), valid_w = carve(words * 8);
        pre_start = carve(words * 4), pre_slot = carve(words * 4), pre_value = carve(words * 4);
        page_starts = carve(npages * 4), page_slots = carve(npages * 4), page_values = carve(npages * 4);
        row0 = carve(npages * 8), slot0 = carve(npages * 8);
        idx = carve(words * 64 * 4);
        sums = carve((csv::scan_tiles_of(npages) + 1) * 8);
        total = carve.at;
    }
};

const char* error_text(unsigned long long err) {
    return err & pqr::kErrLevels   ? "a page's repetition or definition levels are malformed, end early or pass the column's maximum, or a chunk does not begin with a row"
           : err & pqr::kErrIndex  ? "a page's index runs are malformed, end early, or name an entry beyond the dictionary"
           : err & pqr::kErrValues ? "a page is shorter than its values"
                                   : "a row or an element is not where the level words say (did the buffer change during the call?)";
}

template <uint32_t SRC, uint32_t DST, bool FLOAT>
void launch_elements(const PqList& L, void* values, uint8_t* child, unsigned long long* c, hipStream_t st) {
    oxh::pql_elements_kernel<SRC, DST, FLOAT><<<oxh::pq_row_grid(L.nslots), 256, 0, st>>>(L, values, child, c);
}

// Every selected column: measured, and with outputs written into the device buffers the tables name.
int lists_device(ParquetHandle& h, const pqr::ListsArgs& a, bool write, void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity,
                 uint8_t* const* d_child, hipStream_t st) {
    using namespace oxh;
    const uint64_t n = h.nrows();
    uint64_t npages = 0, ndicts = 0, words = 0;
    for (uint32_t k = 0; k < a.nsel; ++k) {
        const pqr::ColumnPages& cp = h.columns[a.col_idx[k]];
        npages = std::max<uint64_t>(npages, cp.lists.size()), ndicts = std::max<uint64_t>(ndicts, cp.dicts.size()), words = std::max(words, cp.words);
    }
    if (npages > 0xFFFFFFFFull) return fail(OXH_ERR_INVALID, "parquet lists: more than 2^32 pages in a column");
    if (csv::scan_tiles_of(npages) != scan_tiles(npages)) return fail(OXH_ERR_HIP, "parquet lists: the scan's tile is not the lease's");
    const ListLease at(a.nsel, npages, ndicts, words);
    ScratchLease lease(st);
    void* lbase = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet lists: " + std::to_string(at.total) + " B of page lists, level words, their counts and indices");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    std::vector<uint32_t> starts(npages), slots(npages);
    int rc = [&]() -> int {
        int r = pq_clear_enqueue(d_ctrl, (uint64_t)a.nsel * pqr::kColWords, st);
        if (r) return r;
        for (uint32_t k = 0; k < a.nsel; ++k) {
            const uint32_t col = a.col_idx[k], type = a.types[k];
            const pqr::ColumnPages& cp = h.columns[col];
            const pqr::Leaf& leaf = h.footer.leaves[col];
            const std::string name = "column '" + leaf.name + "': ";
            const uint32_t np = (uint32_t)cp.lists.size();
            if (!np) return fail(OXH_ERR_INVALID, "parquet lists: " + name + "no data page for the file's " + std::to_string(n) + " rows");
            unsigned long long* c = d_ctrl + (size_t)k * pqr::kColWords;
            PqList L{};
            L.c = PqColumn{h.d_bytes, h.image, (const pqr::DataPage*)(b + at.records), (const pqr::DictPage*)(b + at.dicts), n, np, (uint32_t)cp.dicts.size(), 1u,
                           nullptr, nullptr, (uint32_t*)(b + at.page_values), (uint32_t*)(b + at.idx), nullptr, nullptr, nullptr, nullptr};
            L.lp = (const pqr::ListPage*)(b + at.lp), L.records = (pqr::DataPage*)(b + at.records);
            L.def_list = leaf.def_list, L.def_slot = leaf.def_slot, L.max_def = leaf.max_def, L.width = pqr::level_width(leaf.max_def);
            L.start_w = (uint64_t*)(b + at.start_w), L.slot_w = (uint64_t*)(b + at.slot_w), L.value_w = (uint64_t*)(b + at.value_w), L.valid_w = (uint64_t*)(b + at.valid_w);
            L.pre_start = (uint32_t*)(b + at.pre_start), L.pre_slot = (uint32_t*)(b + at.pre_slot), L.pre_value = (uint32_t*)(b + at.pre_value);
            L.page_starts = (uint32_t*)(b + at.page_starts), L.page_slots = (uint32_t*)(b + at.page_slots);
            L.row0 = (const uint64_t*)(b + at.row0), L.slot0 = (const uint64_t*)(b + at.slot0);
            // the lists are the handle's: they outlive the copies
            HIP_TRY(hipMemcpyAsync(b + at.lp, cp.lists.data(), np * sizeof(pqr::ListPage), hipMemcpyHostToDevice, st));
            if (!cp.dicts.empty()) HIP_TRY(hipMemcpyAsync(b + at.dicts, cp.dicts.data(), cp.dicts.size() * sizeof(pqr::DictPage), hipMemcpyHostToDevice, st));
            pql_levels_kernel<<<pq_wave_grid(np), 256, 0, st>>>(L, c);
            HIP_TRY(hipGetLastError());
            if ((r = exclusive_scan_u32(L.page_starts, np, (uint64_t*)(b + at.row0), (unsigned long long*)(b + at.sums), st))) return r;
            if ((r = exclusive_scan_u32(L.page_slots, np, (uint64_t*)(b + at.slot0), (unsigned long long*)(b + at.sums), st))) return r;
            if (cp.indices && (r = pq_index_enqueue(L.c, c, st))) return r;
            unsigned long long got[pqr::kColWords];
            HIP_TRY(hipMemcpyAsync(starts.data(), L.page_starts, np * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(slots.data(), L.page_slots, np * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(got, c, sizeof got, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (got[pqr::kColErr]) return fail(OXH_ERR_INVALID, "parquet lists: " + name + error_text(got[pqr::kColErr]));
            const std::string rows = pqr::list_rows_error(h.footer, cp, starts.data());
            if (!rows.empty()) return fail(OXH_ERR_INVALID, "parquet lists: " + name + rows);
            for (uint32_t p = 0; p < np; ++p) L.nslots += slots[p];
            const uint32_t cell = pqr::list_cell_bytes(type);
            if (!(type & OXH_PARQUET_LIST64) && L.nslots > 0x7FFFFFFFull)
                return fail(OXH_ERR_INVALID, "parquet lists: " + name + std::to_string(L.nslots) + " elements (int32 offsets hold 2^31 - 1): ask for OXH_PARQUET_LIST64");
            a.value_bytes[k] = L.nslots * cell;
            a.stats4[4 * k] = got[pql::kColNullLists], a.stats4[4 * k + 1] = got[pql::kColNullElements], a.stats4[4 * k + 2] = np + cp.dicts.size();
            a.stats4[4 * k + 3] = L.nslots;
            if (!write) continue;
            if (a.value_bytes[k] > a.value_capacity[k])
                return fail(OXH_ERR_INVALID, "parquet lists: selection " + std::to_string(k) + ": " + std::to_string(a.value_bytes[k]) + " bytes of elements, value_capacity " +
                                                 std::to_string(a.value_capacity[k]));
            if (type & OXH_PARQUET_LIST64)
                pql_rows_kernel<true><<<pq_row_grid(n), 256, 0, st>>>(L, d_offsets[k], d_validity[k], c);
            else
                pql_rows_kernel<false><<<pq_row_grid(n), 256, 0, st>>>(L, d_offsets[k], d_validity[k], c);
            HIP_TRY(hipGetLastError());
            if (!L.nslots) continue;
            if (leaf.physical == pqr::kInt64 || leaf.physical == pqr::kDouble)
                launch_elements<8, 8, false>(L, d_values[k], d_child[k], c, st);
            else if (cell == 4)
                launch_elements<4, 4, false>(L, d_values[k], d_child[k], c, st);
            else if (leaf.physical == pqr::kFloat)
                launch_elements<4, 8, true>(L, d_values[k], d_child[k], c, st);
            else
                launch_elements<4, 8, false>(L, d_values[k], d_child[k], c, st);
            HIP_TRY(hipGetLastError());
            // the next column's level pass reuses the lease: this one's error word comes down first
            HIP_TRY(hipMemcpyAsync(got, c, sizeof got, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (got[pqr::kColErr]) return fail(got[pqr::kColErr] & pqr::kErrValues ? OXH_ERR_INVALID : OXH_ERR_HIP, "parquet lists: " + name + error_text(got[pqr::kColErr]));
        }
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// What both forms do first. `done`: nothing left to do.
int lists_enter(void* handle, pqr::ListsArgs& a, ParquetHandle*& h, bool& done) {
    done = false;
    h = oxh::pq_handle_of(handle);
    if (!h) return fail(OXH_ERR_INVALID, "parquet lists: the handle is NULL or not a Parquet handle");
    a.nrows = h->nrows(), a.ncols = h->ncols();
    const std::string what = pqr::lists_error(a);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet lists: " + what);
    for (uint32_t k = 0; k < a.nsel; ++k) {
        const pqr::Leaf& leaf = h->footer.leaves[a.col_idx[k]];
        const std::string col = "selection " + std::to_string(k) + ", column '" + leaf.name + "': ";
        if (!h->columns[a.col_idx[k]].cause.empty()) return fail(OXH_ERR_INVALID, "parquet lists: " + col + h->columns[a.col_idx[k]].cause);
        if (!leaf.list) return fail(OXH_ERR_INVALID, "parquet lists: " + col + "not a list column: oxh_parquet_columns_* read it");
        if (!pqr::type_fits(leaf.physical, pqr::element_word(a.types[k])))
            return fail(OXH_ERR_INVALID, "parquet lists: " + col + "elements of physical type " + pqr::physical_name(leaf.physical) + " are not read as type " +
                                             std::to_string(pqr::element_word(a.types[k])));
    }
    if (a.nsel == 0 || h->nrows() == 0) {
        for (uint32_t k = 0; k < a.nsel; ++k) a.value_bytes[k] = 0;
        for (uint32_t k = 0; k < 4 * a.nsel; ++k) a.stats4[k] = 0;
        done = true;
        return OXH_OK;
    }
    return oxh::pq_device_enter(h->ctx);
}

}  // namespace

extern "C" {

int oxh_parquet_lists_device(void* parquet, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                             void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity, uint8_t* const* d_child_validity,
                             uint64_t* value_bytes, uint64_t* stats4, void* stream) {
    pqr::ListsArgs a{0, 0, nsel, col_idx, types, value_capacity, d_values, d_offsets, d_validity, d_child_validity, value_bytes, stats4};
    ParquetHandle* h = nullptr;
    bool done = false;
    int rc = lists_enter(parquet, a, h, done);
    if (rc || done) return rc;
    return lists_device(*h, a, d_values != nullptr, d_values, d_offsets, d_validity, d_child_validity, (hipStream_t)stream);
}

int oxh_parquet_lists_host(void* parquet, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                           void* const* values, void* const* offsets, uint8_t* const* validity, uint8_t* const* child_validity,
                           uint64_t* value_bytes, uint64_t* stats4) {
    pqr::ListsArgs a{0, 0, nsel, col_idx, types, value_capacity, values, offsets, validity, child_validity, value_bytes, stats4};
    ParquetHandle* h = nullptr;
    bool done = false;
    int rc = lists_enter(parquet, a, h, done);
    if (rc || done) return rc;
    hipStream_t st = h->ctx->stream;
    if (!values) return lists_device(*h, a, false, nullptr, nullptr, nullptr, nullptr, st);
    // the device block holds what the caller's buffers hold: the elements their value_capacity
    const uint64_t n = h->nrows(), bitmap = (n + 7) / 8;
    std::vector<uint64_t> offset_bytes(nsel), at_values(nsel), at_offsets(nsel), at_validity(nsel), at_child(nsel);
    csv::Carver carve;
    for (uint32_t k = 0; k < nsel; ++k) {
        offset_bytes[k] = (n + 1) * (types[k] & OXH_PARQUET_LIST64 ? 8 : 4);
        at_values[k] = carve(value_capacity[k]), at_offsets[k] = carve(offset_bytes[k]), at_validity[k] = carve(bitmap);
        at_child[k] = carve((value_capacity[k] / pqr::list_cell_bytes(types[k]) + 7) / 8);
    }
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, carve.at + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet lists: " + std::to_string(carve.at) + " B for the columns on the device");
    }
    oxh::poison_device(d_block, carve.at + 16, st);
    std::vector<void*> d_values(nsel), d_offsets(nsel);
    std::vector<uint8_t*> d_validity(nsel), d_child(nsel);
    for (uint32_t k = 0; k < nsel; ++k)
        d_values[k] = d_block + at_values[k], d_offsets[k] = d_block + at_offsets[k], d_validity[k] = d_block + at_validity[k], d_child[k] = d_block + at_child[k];
    rc = [&]() -> int {
        int r = lists_device(*h, a, true, d_values.data(), d_offsets.data(), d_validity.data(), d_child.data(), st);
        if (r) return r;
        // the caller's arrays stay untouched unless everything succeeded
        for (uint32_t k = 0; k < nsel; ++k) {
            const uint64_t elements = stats4[4 * k + 3];
            if (value_bytes[k]) HIP_TRY(hipMemcpyAsync(values[k], d_values[k], value_bytes[k], hipMemcpyDeviceToHost, st));
            if (elements) HIP_TRY(hipMemcpyAsync(child_validity[k], d_child[k], (elements + 7) / 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(offsets[k], d_offsets[k], offset_bytes[k], hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(validity[k], d_validity[k], bitmap, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    return rc;
}

}  // extern "C"
