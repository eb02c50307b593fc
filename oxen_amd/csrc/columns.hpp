// oxen_amd/csrc/columns.hpp -- what the entries over Arrow columns share (row_hash.hip: oxh_row_hashes_*;
// take_columns.hip: oxh_take_columns_*): the kinds, the host forms' staging of a column into one device
// block, and -- for the HIP translation units -- the column descriptor the kernels read and the cell of a
// row. The first half is plain C++ with no HIP in it, so that a stand-alone program can call it
// (tests/native/take_columns_host_test.cpp, which is also what a sanitizer build runs).
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
#include "xxh3_device.hpp"

namespace oxh {

struct RowCol {
    const uint8_t* values;
    const uint8_t* offsets;   // byte columns: nrows + 1 int32 / int64
    const uint8_t* validity;  // NULL: no nulls
    uint64_t vbit;            // OXH_COL_BOOL: the bit of row 0 in values
    uint64_t nbit;            // the bit of row 0 in validity
    uint32_t kind, pad;
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

}  // namespace oxh

namespace oxh::capi {

// A call's small block: the column descriptors and the control words, on the device and pinned.
struct CallBlock {
    uint8_t *d = nullptr, *h = nullptr;
    ~CallBlock() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
    }
    int make(size_t bytes, const char* what) {
        if (hipMalloc(&d, bytes) != hipSuccess || hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, std::string(what) + ": control block");
        }
        memset(h, 0, bytes);
        return OXH_OK;
    }
};

}  // namespace oxh::capi
#endif  // __HIPCC__
