// oxen_amd/csrc/embedding_host.hpp -- the host-only pieces of oxh_embedding_* (embedding.hip): the column of
// vectors as the three entries describe it, what both forms check before they need a device, the descending
// order key of a similarity (sort_keys.hpp's float word, inverted), the partition of the mean, the page
// arithmetic and the host forms' staging plan (one device block that holds only the span the named rows
// name). Plain C++ with no HIP in it, so that a stand-alone program can call it
// (tests/native/embedding_host_test.cpp, which is also what a sanitizer build runs).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/oxen_hash.h"
#include "sort_keys.hpp"

namespace oxh::embedding {

constexpr uint64_t kMaxRows = 0xFFFFFFFEull;   // row indices are u32, and usable as the take's idx0
constexpr uint32_t kNullKey = 0xFFFFFFFFu;     // the order key of a null similarity: after every valid key

inline bool known_layout(uint32_t layout) { return layout == OXH_EMB_FIXED || layout == OXH_EMB_LIST32 || layout == OXH_EMB_LIST64; }
inline bool is_list(uint32_t layout) { return layout == OXH_EMB_LIST32 || layout == OXH_EMB_LIST64; }
inline uint32_t offset_width(uint32_t layout) { return layout == OXH_EMB_LIST32 ? 4 : 8; }
inline int64_t offset_at(const void* offsets, uint32_t layout, uint64_t r) {
    return layout == OXH_EMB_LIST32 ? (int64_t)((const int32_t*)offsets)[r] : ((const int64_t*)offsets)[r];
}

// The descending order of similarities as an ascending unsigned key: the bitwise NOT of the sort's float word.
// NaN (one word, above +inf) comes first, then +1 .. -1 with -0.0 equal to +0.0; the largest valid key is that
// of -inf, 0xFF800000, so kNullKey is no valid row's key.
OXH_SORT_HD uint32_t order_key(uint32_t sim_bits) { return ~(uint32_t)sortkeys::encode_float32(sim_bits); }

// One column of vectors, as every entry takes it.
struct Column {
    uint32_t layout;
    uint64_t nrows;
    uint32_t dim;
    const void* values;      // float32, 4-byte aligned
    const void* offsets;     // the list layouts: nrows + 1 int32 / int64, in elements of values
    const uint8_t* validity; // may be NULL
    uint64_t validity_bit;
};

// What is wrong with the column ("" when nothing is), in the header's order. host: the offsets can be read.
inline std::string column_error(const Column& c, bool host) {
    if (!known_layout(c.layout)) return "unknown layout " + std::to_string(c.layout);
    if (c.dim == 0) return "dim is 0";
    if (c.nrows > kMaxRows) return "more than 2^32 - 2 rows";
    if (c.nrows == 0) return "";
    if (((uintptr_t)c.values & 3) != 0) return "values is not 4-byte aligned";
    if (!is_list(c.layout)) return c.values ? "" : "the column has rows but no values";
    if (!c.offsets) return "a list column without offsets";
    if (!host) return c.values ? "" : "the column has rows but no values";
    int64_t before = offset_at(c.offsets, c.layout, 0);
    if (before < 0) return "offsets[0] is negative";
    const int64_t lo = before;
    for (uint64_t r = 1; r <= c.nrows; ++r) {
        const int64_t at = offset_at(c.offsets, c.layout, r);
        if (at < before) return "offsets decrease at row " + std::to_string(r - 1);
        before = at;
    }
    if (!c.values && before > lo) return "the column has elements but no values";
    return "";
}

struct MeanArgs {
    Column col;
    const uint32_t* idx;
    uint64_t nidx;
    void* out;
    uint64_t* stats4;
};
inline std::string mean_error(const MeanArgs& a, bool host) {
    const std::string what = column_error(a.col, host);
    if (!what.empty()) return what;
    if (a.nidx > kMaxRows) return "more than 2^32 - 2 indices";
    if (a.col.nrows && a.nidx && !a.idx) return "idx is NULL";
    if (a.col.nrows && a.nidx && !a.out) return "out is NULL";
    if (!a.stats4) return "stats4 is NULL";
    if (host && a.col.nrows)
        for (uint64_t i = 0; i < a.nidx; ++i)
            if (a.idx[i] >= a.col.nrows) return "idx[" + std::to_string(i) + "] = " + std::to_string(a.idx[i]) + " is not a row of " + std::to_string(a.col.nrows);
    return "";
}

struct SimilarityArgs {
    Column col;
    const void* query;
    void* sim;
    uint8_t* sim_validity;   // may be NULL when the column has no validity
    uint32_t* order_key;     // may be NULL
    uint32_t* perm;          // may be NULL; needs order_key
    uint64_t* stats4;
};
inline std::string similarity_error(const SimilarityArgs& a, bool host) {
    const std::string what = column_error(a.col, host);
    if (!what.empty()) return what;
    if (a.perm && !a.order_key) return "perm needs order_key";
    if (a.col.nrows) {
        if (!a.query) return "query is NULL";
        if (!a.sim) return "sim is NULL";
        if (a.col.validity && !a.sim_validity) return "the column has a validity bitmap and sim_validity is NULL";
    }
    if (!a.stats4) return "stats4 is NULL";
    return "";
}

struct TakeArgs {
    Column col;
    const uint32_t* idx;
    uint64_t nout;
    void* out_values;
    uint8_t* out_validity;
    uint64_t* stats4;
};
inline std::string take_error(const TakeArgs& a, bool host) {
    // a take of no rows from a column of no rows is fine; the column is looked at only when it has rows
    const std::string what = column_error(a.col, host);
    if (!what.empty()) return what;
    if (a.nout > kMaxRows) return "more than 2^32 - 2 output rows";
    if (a.nout && (!a.idx || !a.out_values || !a.out_validity)) return "idx, out_values or out_validity is NULL";
    if (!a.stats4) return "stats4 is NULL";
    if (host)
        for (uint64_t i = 0; i < a.nout; ++i)
            if (a.idx[i] != OXH_TAKE_NULL && a.idx[i] >= a.col.nrows)
                return "idx[" + std::to_string(i) + "] = " + std::to_string(a.idx[i]) + " is neither absent nor a row of " + std::to_string(a.col.nrows);
    return "";
}

// ---------------------------------------------------------------- the mean's partition
// The selected rows are cut into chunks of kMeanChunk neighbouring idx entries; workgroup g of G adds the chunks
// g, g + G, .. in that order. G depends on nidx alone, so the partial sums and the order they are added in do
// not change from run to run or between the two forms.
constexpr uint32_t kMeanChunk = 64, kMeanMaxGroups = 1024;
inline uint32_t mean_groups(uint64_t nidx) {
    const uint64_t chunks = (nidx + kMeanChunk - 1) / kMeanChunk;
    return (uint32_t)(chunks < 1 ? 1 : chunks > kMeanMaxGroups ? kMeanMaxGroups : chunks);
}
// lanes of a 256-lane workgroup across dim: the smallest power of two that holds dim, at most 256
inline uint32_t mean_lanes(uint32_t dim) {
    uint32_t lanes = 1;
    while (lanes < dim && lanes < 256) lanes *= 2;
    return lanes;
}
inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
constexpr uint64_t kCtrlBytes = 256;   // the control words of a call
// the device scratch of a mean: the control words, then mean_groups(nidx) x dim partial sums
inline uint64_t mean_lease_bytes(uint64_t nidx, uint32_t dim) { return kCtrlBytes + align256((uint64_t)mean_groups(nidx) * dim * 4); }

// ---------------------------------------------------------------- a page of the ranked rows
// `LIMIT page_size OFFSET (page_num - 1) * page_size` over nrows ranked rows: [first, first + count), clipped to
// the frame; page_num 0 is page 1.
struct Page {
    uint64_t first, count;
};
inline Page page_of(uint64_t nrows, uint64_t page_size, uint64_t page_num) {
    const uint64_t page = page_num ? page_num - 1 : 0;
    if (page_size == 0 || page > nrows / page_size) return Page{nrows, 0};
    const uint64_t first = page * page_size;
    if (first >= nrows) return Page{nrows, 0};
    return Page{first, page_size < nrows - first ? page_size : nrows - first};
}

// ---------------------------------------------------------------- the host forms' device block
// One block for what a call copies up and what it brings back. Of the column only the rows [row_lo, row_hi)
// are there: their floats (a list column: the span [offsets[row_lo], offsets[row_hi])), their offsets and the
// bytes that hold their validity bits. The floats keep the caller's phase within 16 bytes, so that both forms
// take the same loads. The kernels address a row relative to row_lo and an element relative to elem_lo.
struct Piece {
    const void* src;   // NULL: room for an output
    uint64_t bytes, at;
};

struct HostPlan {
    std::vector<Piece> pieces;
    uint64_t total = 0;
    uint64_t row_lo = 0, row_hi = 0, elem_lo = 0, elem_hi = 0;
    int64_t values = -1, offsets = -1, validity = -1;
    uint64_t nbit = 0;   // the bit of row_lo in the staged validity

    int64_t add(const void* src, uint64_t bytes, uint64_t phase = 0) {
        pieces.push_back({src, bytes, total + phase});
        total += (phase + bytes + 15) & ~15ull;
        return (int64_t)pieces.size() - 1;
    }
    // c passed column_error(host = true); row_lo <= row_hi <= nrows
    void add_column(const Column& c, uint64_t lo, uint64_t hi) {
        row_lo = lo, row_hi = hi;
        if (hi <= lo) return;
        if (is_list(c.layout)) {
            elem_lo = (uint64_t)offset_at(c.offsets, c.layout, lo), elem_hi = (uint64_t)offset_at(c.offsets, c.layout, hi);
            offsets = add((const uint8_t*)c.offsets + lo * offset_width(c.layout), (hi - lo + 1) * offset_width(c.layout));
        } else {
            elem_lo = lo * c.dim, elem_hi = hi * c.dim;
        }
        if (elem_hi > elem_lo) {
            const uint8_t* src = (const uint8_t*)c.values + 4 * elem_lo;
            values = add(src, 4 * (elem_hi - elem_lo), (uintptr_t)src & 15);
        }
        if (c.validity) {
            const uint64_t bit = c.validity_bit + lo;
            nbit = bit & 7;
            validity = add(c.validity + (bit >> 3), (nbit + (hi - lo) + 7) >> 3);
        }
    }
    uint8_t* at(uint8_t* block, int64_t piece) const { return piece < 0 ? nullptr : block + pieces[piece].at; }
};

}  // namespace oxh::embedding
