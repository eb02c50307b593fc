// oxen_amd/csrc/parquet_device.hpp -- what the Parquet writer's kernels share (parquet_write.hip: measure and emit;
// parquet_dict.hip: the dictionary chunks of OXH_PARQUET_DICTIONARY; parquet_write_lists.hip: the list columns): the
// column table and the plan as the kernels read them, the rank of a row inside a ballot, the staged store and the
// straight copy on the destination's 16-byte grid, and the dictionary and list steps as the writer's call enqueues them.
#pragma once

#include "capi_internal.hpp"
#include "columns.hpp"
#include "parquet_host.hpp"

namespace oxh {

constexpr uint32_t kPqSpanLds = 8192;      // a wave's LDS: one tile of 8-byte cells, or a run of string cells
constexpr unsigned kPqMaxGroups = 1024;    // workgroups of a launch (4 of 32 KiB LDS fill a CU); the rest by grid stride
constexpr unsigned long long kPqErrCell = 4, kPqErrPlace = 8;  // beside kRowErrOffsets, kRowErrValues
constexpr int kPqErr = 0, kPqCtrlWords = 8;

struct PqCol {
    RowCol c;
    uint32_t type;  // OXH_CSV_*
    uint32_t pad;
};

struct PqArgs {
    const PqCol* cols;
    uint64_t nrows, ntiles;
    uint32_t ncols;
};

struct PqEmit {
    const parquet::Page* pages;
    const parquet::Place* places;
    const uint8_t* blob;
    uint64_t npages;
    uint8_t* out;
};

__device__ __forceinline__ bool pqw_present(const RowCol& c, uint64_t r) { return !c.validity || row_bit(c.validity, c.nbit + r); }
// The set bits of a ballot below this lane.
__device__ __forceinline__ uint32_t pqw_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

typedef uint32_t PqBlock16 __attribute__((ext_vector_type(4)));  // one 16-byte block
// The output is global memory; saying so keeps the stores off the flat path.
#define OXH_PQW_GLOBAL __attribute__((address_space(1)))

// The writer's LDS is private to a wave, whose LDS operations execute in order: the fences only keep the
// compiler from moving them across (they emit no instruction).
__device__ __forceinline__ void pqw_wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The n <= kPqSpanLds bytes staged from stage[d & 15] on to d[0 .. n): 16 bytes a lane on d's 16-byte grid, the
// blocks that hold the span's head or tail byte by byte.
__device__ __forceinline__ void pqw_store_span(uint8_t* d, uint64_t n, const uint8_t* stage, unsigned lane) {
    const uintptr_t d0 = (uintptr_t)d, d1 = d0 + n, grid0 = d0 & ~(uintptr_t)15;
    for (uint32_t b = 16 * lane; grid0 + b < d1; b += 16 * 64) {
        const uintptr_t to = grid0 + b;
        if (to >= d0 && to + 16 <= d1) {
            *(OXH_PQW_GLOBAL PqBlock16*)to = *(const PqBlock16*)&stage[b];
        } else {
            for (uint32_t k = 0; k < 16; ++k)
                if (to + k >= d0 && to + k < d1) *(OXH_PQW_GLOBAL uint8_t*)(to + k) = stage[b + k];
        }
    }
}

// n bytes from src (any alignment) to d, without LDS: each lane loads the 16 source bytes that fall on one block of
// d's 16-byte grid and stores the block; the blocks that hold the span's head or tail go byte by byte.
__device__ __forceinline__ void pqw_copy_span(uint8_t* d, const uint8_t* src, uint64_t n, unsigned lane) {
    const uintptr_t d0 = (uintptr_t)d, d1 = d0 + n, grid0 = d0 & ~(uintptr_t)15;
    for (uint64_t b = 16 * lane; grid0 + b < d1; b += 16 * 64) {
        const uintptr_t to = grid0 + b;
        if (to >= d0 && to + 16 <= d1) {
            PqBlock16 v;
            __builtin_memcpy(&v, src + (to - d0), 16);
            *(OXH_PQW_GLOBAL PqBlock16*)to = v;
        } else {
            for (uint32_t k = 0; k < 16; ++k)
                if (to + k >= d0 && to + k < d1) *(OXH_PQW_GLOBAL uint8_t*)(to + k) = src[to + k - d0];
        }
    }
}

// ---------------------------------------------------------------- OXH_PARQUET_DICTIONARY (parquet_dict.hip)
// The dictionary steps of one writer call, in the call's lease behind its plan. build(), after the measure kernel on
// the same stream: the distinct values of every candidate chunk (a row group's INT64, DOUBLE or string column) and
// their first-occurrence ranks; d_chunks[group * ncols + column] is then what the planner reads. write(), after the
// emit kernel: the dictionary pages' entries, every valid row's index in a dense array, and the bit-packed runs.
struct PqdPack {  // per data page of a dictionary chunk, in the order of dense_at: where its indices start, and the page
    uint64_t dense_at;
    uint32_t page, pad;
};

struct PqDict {
    // the device working memory of a call over these columns, 0 when no column is a candidate
    static uint64_t work_bytes(uint64_t nrows, uint32_t ncols, const uint32_t* types, uint64_t group_rows);
    int build(const PqArgs& args, const uint32_t* types, uint64_t group_rows, uint8_t* d_work, parquet::ChunkDict* d_chunks,
              unsigned long long* d_ctrl, hipStream_t st);
    int write(const PqArgs& args, const PqEmit& em, const parquet::Plan& plan, unsigned long long* d_ctrl, hipStream_t st);

    uint32_t ncand = 0, nstr = 0, slots = 0;
    uint64_t group_rows = 0, ngroups = 0, nflat = 0, nflat_str = 0;
    uint8_t* d_work = nullptr;
    uint64_t at_cand = 0, at_tables = 0, at_count = 0, at_slot = 0, at_dense = 0, at_place = 0, at_sums = 0, at_strlen = 0, at_strplace = 0,
             at_strsums = 0, at_packs = 0, total = 0;
    std::vector<uint32_t> cand;   // what goes up: they live until the call's stream has drained
    std::vector<PqdPack> packs;
    void layout(uint64_t nrows, uint32_t ncols, const uint32_t* types, uint64_t group_rows);
};

// ---------------------------------------------------------------- list columns (parquet_write_lists.hip)
constexpr unsigned long long kPqErrListLong = 16, kPqErrListValues = 32, kPqErrListOffsets = 64;  // beside kPqErrCell, kPqErrPlace
constexpr uint32_t kPqlBlockEntries = 4096;  // the level entries of a page that one wave emits at a time

// One list column as its kernels read it: the Arrow arrays, then the call's scratch over its rows and, once the
// entries are counted, over its 64-entry words.
struct PqListCol {
    RowCol c;              // values: the elements; offsets: the lists' nrows + 1; validity, nbit: the lists' bitmap
    const uint8_t* child;  // the elements' bitmap; NULL: no null element
    uint64_t cbit;         // the bit of element elem_lo in it
    uint64_t elem_lo;      // the element that values[0] holds (the host form stages only the span its lists name)
    uint32_t col, width, wide, pad;  // its column; an element's bytes; int64 offsets
    uint32_t* count;       // nrows + 1: a row's level entries, the last 0
    uint64_t* entry0;      // nrows + 1: the entries in front of a row; the last is `total`
    uint64_t total, nwords;
    uint64_t* words[4];    // per 64 entries: the repetition bits, definition bit 0, definition bit 1, def == 3
    uint32_t* vcount;      // nwords + 1: the popcount of words[3], the last 0
    uint64_t* vbase;       // nwords + 1: the values in front of a word; the last is the column's values
};

struct PqlItem {  // block `block` of kPqlBlockEntries entries of page `page`
    uint32_t page, block;
};

// The list steps of one writer call. measure(), behind the measure kernel on the same stream: the entries per row and
// their scan, the level words and their value ranks, then the list columns' entries of the tile table (Tile: min = the
// tile's entries, value_bytes = its values' bytes, valid = its lists that are not null). It synchronises once in the
// middle, because the entry totals size the words. emit(), behind the emit kernel: the list pages' heads, level
// streams and values. The two blocks of working memory are the call's own.
struct PqLists {
    ~PqLists();
    int measure(const PqArgs& args, const uint32_t* types, const PqCol* h_cols, const uint8_t* const* d_child, const uint64_t* child_bits,
                const uint64_t* elem_lo, parquet::Tile* d_tiles, unsigned long long* d_ctrl, unsigned long long* h_ctrl, hipStream_t st);
    int emit(const PqEmit& em, const parquet::Plan& plan, unsigned long long* d_ctrl, hipStream_t st);

    std::vector<PqListCol> cols;
    std::vector<PqlItem> items;  // what goes up: it lives until the call's stream has drained
    std::vector<uint64_t> items_at;  // per list column: where its items lie in d_words
    uint64_t ntiles = 0;
    uint8_t *d_rows = nullptr, *d_words = nullptr;
    // OXH_TRACE: the steps' events and the host's clock (parquet_write_lists.hip)
    bool trace = false;
    hipEvent_t ev[8] = {};
    double host_ms[3] = {};
    void mark(int k, hipStream_t st);
};

}  // namespace oxh
