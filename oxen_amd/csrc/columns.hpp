// oxen_amd/csrc/columns.hpp -- what the entries over Arrow columns share (row_hash.hip: oxh_row_hashes_*;
// take_columns.hip: oxh_take_columns_*; sort_rows.hip: oxh_sort_rows_*; group_rows.hip: oxh_group_rows_*): the
// kinds, the host forms' staging of a column into one device block, and -- for the HIP translation units -- the
// column descriptor the kernels read, the cell of a row, what a cell adds to a row's image (the raw one of the
// row hashes, the keyed one of the grouping) and the call that hashes those images. The first half is plain
// C++ with no HIP in it, so that a stand-alone program can call it (tests/native/take_columns_host_test.cpp,
// which is also what a sanitizer build runs).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/oxen_hash.h"

namespace oxh::cols {

inline bool is_bytes(uint32_t kind) { return kind == OXH_COL_BYTES32 || kind == OXH_COL_BYTES64; }
inline bool known_kind(uint32_t kind) {
    return kind == OXH_COL_FIXED1 || kind == OXH_COL_FIXED4 || kind == OXH_COL_FIXED8 || kind == OXH_COL_BOOL || is_bytes(kind);
}
// bytes of one cell of a fixed-width column (OXH_COL_FIXED* are their widths); 0 for the other kinds
inline uint32_t width_of(uint32_t kind) {
    return kind == OXH_COL_FIXED1 || kind == OXH_COL_FIXED4 || kind == OXH_COL_FIXED8 ? kind : 0;
}
inline uint32_t offset_width(uint32_t kind) { return kind == OXH_COL_BYTES32 ? 4 : 8; }

inline int64_t offset_at(const void* offsets, uint32_t kind, uint64_t r) {
    return kind == OXH_COL_BYTES32 ? (int64_t)((const int32_t*)offsets)[r] : ((const int64_t*)offsets)[r];
}

// What is wrong with one column of `nrows` > 0 rows ("" when nothing is): NULL offsets of a byte column,
// NULL values of any other; host (the offsets can be read): offsets that are negative or decrease, bytes
// without values. `col` starts the message ("row hashes: column 3").
inline std::string column_error(const std::string& col, uint32_t kind, const void* values, const void* offsets, uint64_t nrows,
                                bool host) {
    if (!is_bytes(kind)) return values ? "" : col + " has no values";
    if (!offsets) return col + " is a byte column without offsets";
    if (!host) return "";  // the spans are on the device: the kernels check them
    int64_t before = offset_at(offsets, kind, 0);
    if (before < 0) return col + ": offsets[0] is negative";
    const int64_t lo = before;
    for (uint64_t r = 1; r <= nrows; ++r) {
        const int64_t at = offset_at(offsets, kind, r);
        if (at < before) return col + ": offsets decrease at row " + std::to_string(r - 1);
        before = at;
    }
    if (!values && before > lo) return col + " has bytes but no values";
    return "";
}

// The host forms' staging plan: one device block that holds, for every column, only what its rows name --
// nrows values (the bytes that hold its bits for a boolean), the nrows + 1 offsets and the span
// [offsets[0], offsets[nrows]) of a byte column, the bytes that hold its validity bits -- each piece 16-B
// aligned. Nothing here touches a device: `pieces` says what to copy where, the *_at functions where a
// column's arrays are once the block has an address.
struct Piece {
    const void* src;
    uint64_t bytes, at;
};

struct Staged {              // one column's pieces (-1: none) and what the kernels get beside the pointers
    int64_t values = -1, offsets = -1, validity = -1;
    uint64_t span_lo = 0;    // a byte column's offsets[0]: its values piece starts at that byte of the caller's buffer
    uint64_t vbit = 0, nbit = 0;  // the residual bit offsets
};

struct Staging {
    std::vector<Piece> pieces;
    uint64_t total = 0;      // bytes of the block so far; a caller may reserve the front by starting above 0

    int64_t add(const void* src, uint64_t bytes) {
        pieces.push_back({src, bytes, total});
        total += (bytes + 15) & ~15ull;
        return (int64_t)pieces.size() - 1;
    }
    int64_t add_bits(const uint8_t* src, uint64_t bit0, uint64_t nrows, uint64_t& bit_out) {
        bit_out = bit0 & 7;
        return add(src + (bit0 >> 3), (bit_out + nrows + 7) >> 3);
    }
    // A column of nrows > 0 rows whose arrays passed column_error(host = true).
    Staged add_column(uint32_t kind, const void* values, const void* offsets, const uint8_t* validity, uint64_t value_bit,
                      uint64_t validity_bit, uint64_t nrows) {
        Staged s;
        if (kind == OXH_COL_BOOL) {
            s.values = add_bits((const uint8_t*)values, value_bit, nrows, s.vbit);
        } else if (!is_bytes(kind)) {
            s.values = add(values, nrows * width_of(kind));
        } else {
            const uint64_t lo = (uint64_t)offset_at(offsets, kind, 0), hi = (uint64_t)offset_at(offsets, kind, nrows);
            s.span_lo = lo;
            s.offsets = add(offsets, (nrows + 1) * offset_width(kind));
            if (hi > lo) s.values = add((const uint8_t*)values + lo, hi - lo);
        }
        if (validity) s.validity = add_bits(validity, validity_bit, nrows, s.nbit);
        return s;
    }
    // A byte column's values pointer is where byte 0 of the caller's buffer would be: the kernels add the
    // offsets as they are, and only [offsets[0], offsets[nrows]) is ever read.
    const void* values_at(const uint8_t* block, const Staged& s) const {
        return s.values < 0 ? nullptr : (const void*)((uintptr_t)(block + pieces[s.values].at) - (uintptr_t)s.span_lo);
    }
    const void* offsets_at(const uint8_t* block, const Staged& s) const {
        return s.offsets < 0 ? nullptr : block + pieces[s.offsets].at;
    }
    const uint8_t* validity_at(const uint8_t* block, const Staged& s) const {
        return s.validity < 0 ? nullptr : block + pieces[s.validity].at;
    }
};

}  // namespace oxh::cols

#if defined(__HIPCC__)
#include "sort_keys.hpp"
#include "xxh3_device.hpp"

namespace oxh {

struct RowCol {
    const uint8_t* values;
    const uint8_t* offsets;   // byte columns: nrows + 1 int32 / int64
    const uint8_t* validity;  // NULL: no nulls
    uint64_t vbit;            // OXH_COL_BOOL: the bit of row 0 in values
    uint64_t nbit;            // the bit of row 0 in validity
    uint32_t kind;
    uint32_t order;           // OXH_SORT_* of a fixed-width column in a key image (image_cell below); else unused
};

constexpr unsigned long long kRowErrOffsets = 1, kRowErrValues = 2;

__device__ __forceinline__ bool row_bit(const uint8_t* p, uint64_t bit) { return (p[bit >> 3] >> (bit & 7)) & 1; }

// Length of row r's cell in column c; byte columns: `start` = where its bytes begin in c.values.
__device__ __forceinline__ uint64_t row_cell(const RowCol& c, uint64_t r, uint64_t& start, unsigned long long& bad) {
    if (c.validity && !row_bit(c.validity, c.nbit + r)) return 0;
    switch (c.kind) {
        case OXH_COL_FIXED1:
        case OXH_COL_BOOL: return 1;
        case OXH_COL_FIXED4: return 4;
        case OXH_COL_FIXED8: return 8;
        default: break;
    }
    int64_t s, e;
    if (c.kind == OXH_COL_BYTES32) {
        s = (int32_t)ld32u(c.offsets + 4 * r);
        e = (int32_t)ld32u(c.offsets + 4 * r + 4);
    } else {
        s = (int64_t)ld64u(c.offsets + 8 * r);
        e = (int64_t)ld64u(c.offsets + 8 * r + 8);
    }
    if (s < 0 || e < s) {  // never a read through such a pair
        bad |= kRowErrOffsets;
        return 0;
    }
    if (e > s && !c.values) {
        bad |= kRowErrValues;
        return 0;
    }
    start = (uint64_t)s;
    return (uint64_t)(e - s);
}

// ---------------------------------------------------------------- a row's image, cell by cell
// What a cell adds to the image of its row that a lane (or a wave) assembles and hashes. Two images:
//   raw    (KEYED = false; the row hashes, row_hash.hip) nothing for a null, else the cell's bytes: the
//          reference's any_val_to_bytes, cells not delimited;
//   keyed  (KEYED = true; the grouping, group_rows.hip) one tag byte, 0 for a null and 1 for a present cell; then
//          -- fixed-width: the w low bytes of sort_keys.hpp's word of the cell, a bijection of the cell's bytes
//          but under OXH_SORT_FLOAT, where -0.0 and +0.0 share a word and all NaNs another; boolean: one byte 0 /
//          1; byte cell: its length, little endian in the width of the column's offsets, then its bytes. No
//          cell's encoding is a prefix of another's of the same column, so the concatenation over the columns
//          is injective over rows, and rows equal under the grouping's equality have one image.
struct ImageCell {
    uint64_t start;   // byte cells: where the bytes begin in the column's values
    uint64_t len;     // the cell's own bytes (row_cell: 0 for a null, and for a bad pair of offsets)
    uint32_t head;    // keyed: the bytes in front of them (the tag, a byte cell's length)
    bool present;     // keyed: not a null
};

// The bytes row r's cell of column c adds to the image; `cell` says where they come from.
template <bool KEYED>
__device__ __forceinline__ uint64_t image_cell(const RowCol& c, uint64_t r, ImageCell& cell, unsigned long long& bad) {
    cell.start = 0;
    cell.len = row_cell(c, r, cell.start, bad);
    cell.head = 0;
    cell.present = true;
    if constexpr (KEYED) {
        cell.present = !c.validity || row_bit(c.validity, c.nbit + r);
        cell.head = !cell.present ? 1 : c.kind == OXH_COL_BYTES32 ? 5 : c.kind == OXH_COL_BYTES64 ? 9 : 1;
    }
    return cell.head + cell.len;
}

// Exactly the n bytes of a span, by one lane: the widest pieces first.
__device__ __forceinline__ void copy_span_lane(uint8_t* dst, const uint8_t* src, uint32_t n) {
    uint32_t b = 0;
    for (; b + 8 <= n; b += 8) {
        const uint64_t v = ld64u(src + b);
        __builtin_memcpy(dst + b, &v, 8);
    }
    if (b + 4 <= n) {
        const uint32_t v = ld32u(src + b);
        __builtin_memcpy(dst + b, &v, 4);
        b += 4;
    }
    for (; b < n; ++b) dst[b] = src[b];
}

// Exactly the n bytes of a span, by the 64 lanes of a wave: whole 8-byte pieces across the lanes (512 B per
// wave-instruction, any alignment), then the last n % 8 bytes one lane each.
__device__ __forceinline__ void copy_span_wave(uint8_t* dst, const uint8_t* src, uint64_t n, unsigned lane) {
    const uint64_t whole = n & ~7ull;
    for (uint64_t b = 8ull * lane; b < whole; b += 512) {
        const uint64_t v = ld64u(src + b);
        __builtin_memcpy(dst + b, &v, 8);
    }
    if (whole + lane < n) dst[whole + lane] = src[whole + lane];
}

// The low `width` bytes of v, little endian.
__device__ __forceinline__ void put_word(uint8_t* dst, uint64_t v, uint32_t width) {
    if (width == 8) {
        __builtin_memcpy(dst, &v, 8);
    } else if (width == 4) {
        const uint32_t w = (uint32_t)v;
        __builtin_memcpy(dst, &w, 4);
    } else {
        dst[0] = (uint8_t)v;
    }
}

// A keyed cell but for a byte cell's bytes: the tag, then a fixed-width cell's word, a boolean's byte, a byte
// cell's length.
__device__ __forceinline__ void put_keyed_head(uint8_t* dst, const RowCol& c, uint64_t r, const ImageCell& cell) {
    dst[0] = cell.present ? 1 : 0;
    if (!cell.present) return;
    switch (c.kind) {
        case OXH_COL_FIXED1: put_word(dst + 1, sortkeys::fixed_word(c.order, 1, c.values[r]), 1); break;
        case OXH_COL_FIXED4: put_word(dst + 1, sortkeys::fixed_word(c.order, 4, ld32u(c.values + 4 * r)), 4); break;
        case OXH_COL_FIXED8: put_word(dst + 1, sortkeys::fixed_word(c.order, 8, ld64u(c.values + 8 * r)), 8); break;
        case OXH_COL_BOOL: dst[1] = row_bit(c.values, c.vbit + r) ? 1 : 0; break;
        default: put_word(dst + 1, cell.len, c.kind == OXH_COL_BYTES32 ? 4 : 8); break;
    }
}

// The cell (image_cell's) to dst, by one lane.
template <bool KEYED>
__device__ __forceinline__ void image_put_lane(uint8_t* dst, const RowCol& c, uint64_t r, const ImageCell& cell) {
    if constexpr (KEYED) {
        put_keyed_head(dst, c, r, cell);
        if (cell.len && (c.kind == OXH_COL_BYTES32 || c.kind == OXH_COL_BYTES64))
            copy_span_lane(dst + cell.head, c.values + cell.start, (uint32_t)cell.len);
    } else {
        if (cell.len == 0) return;
        switch (c.kind) {
            case OXH_COL_FIXED1: dst[0] = c.values[r]; break;
            case OXH_COL_BOOL: dst[0] = row_bit(c.values, c.vbit + r) ? 1 : 0; break;
            case OXH_COL_FIXED4: put_word(dst, ld32u(c.values + 4 * r), 4); break;
            case OXH_COL_FIXED8: put_word(dst, ld64u(c.values + 8 * r), 8); break;
            default: copy_span_lane(dst, c.values + cell.start, (uint32_t)cell.len); break;
        }
    }
}

// The cell to dst, by the lanes of one wave (every lane calls it).
template <bool KEYED>
__device__ __forceinline__ void image_put_wave(uint8_t* dst, const RowCol& c, uint64_t r, const ImageCell& cell, unsigned lane) {
    const bool bytes = c.kind == OXH_COL_BYTES32 || c.kind == OXH_COL_BYTES64;
    if constexpr (KEYED) {
        if (lane == 0) put_keyed_head(dst, c, r, cell);
        if (bytes && cell.len) copy_span_wave(dst + cell.head, c.values + cell.start, cell.len, lane);
    } else {
        if (c.kind == OXH_COL_BOOL) {
            if (cell.len && lane == 0) dst[0] = row_bit(c.values, c.vbit + r) ? 1 : 0;
        } else {
            copy_span_wave(dst, c.values + (bytes ? cell.start : r * cell.len), cell.len, lane);
        }
    }
}

}  // namespace oxh

namespace oxh::capi {

// A call's small block: the column descriptors and the control words, on the device and pinned.
struct CallBlock {
    uint8_t *d = nullptr, *h = nullptr;
    ~CallBlock() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
    }
    // `st`: the stream the call's work on the block is queued on. The pinned half comes back zeroed -- the callers
    // count on that for the control words they send up -- so of a poison (scratch.hpp) only the device half's stays.
    int make(size_t bytes, const char* what, hipStream_t st) {
        if (hipMalloc(&d, bytes) != hipSuccess || hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, std::string(what) + ": control block");
        }
        oxh::poison_device(d, bytes, st);
        oxh::poison_pinned(h, bytes);
        memset(h, 0, bytes);
        return OXH_OK;
    }
};

// The digests of every row's image over device-resident columns (row_hash.hip), in two steps so that a caller
// can keep the long rows' scratch inside a lease of its own (leases do not nest):
//   measure  the column descriptors go up, the length pass runs; then longest / nlong / long_bytes are known;
//   hash     the short rows' kernel, and the long path inside `scratch` (scratch_bytes() of device memory that
//            nobody else touches until the call returns; not read when that is 0); complete on return.
// keyed: the grouping's key image (image_cell above; orders[c] = OXH_SORT_* of a fixed-width column) in place of
// the raw one. A bad pair of offsets is a cell of length 0 in either; the raw form returns OXH_ERR_INVALID at
// once, the keyed form finishes first -- d_out then holds the digests of the frame with that cell empty.
struct RowImageCall {
    CallBlock block;
    size_t ctrl_at = 0;
    bool keyed = false, gather_all = false;
    uint64_t nrows = 0, longest = 0, nlong = 0, long_bytes = 0;
    uint32_t ncols = 0, short_max = 0;
    int deferred = OXH_OK;  // keyed: what a bad cell makes the call return in the end
    int measure(bool keyed_image, uint64_t rows, uint32_t cols, const uint32_t* kinds, const uint32_t* orders,
                const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                const uint64_t* bit_offsets, hipStream_t st);
    uint64_t scratch_bytes() const;
    int hash(uint64_t* d_out, void* scratch, hipStream_t st);
};

}  // namespace oxh::capi
#endif  // __HIPCC__
