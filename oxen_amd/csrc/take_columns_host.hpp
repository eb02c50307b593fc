// oxen_amd/csrc/take_columns_host.hpp -- the host-only pieces of oxh_take_columns_* (take_columns.hip): what
// both forms check before they need a device, the sizes the host knows without one, and the host form's
// output block. Plain C++ with no HIP in it, so that a stand-alone program can call it
// (tests/native/take_columns_host_test.cpp, which is also what a sanitizer build runs). The staging of
// the source columns is columns.hpp's.
#pragma once

#include "columns.hpp"

namespace oxh::take {

constexpr uint64_t kMaxRows = 0xFFFFFFFEull;   // row indices are u32 and 0xFFFFFFFF is "absent"
constexpr uint64_t kMaxBytes32 = 0x7FFFFFFFull;  // what an int32 offset can say

struct Args {
    uint32_t nsrc;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint64_t* src_rows;
    uint64_t nout_rows;
    const uint32_t *idx0, *idx1;
    uint32_t nout;
    const uint32_t* plan;
    const uint64_t* value_capacity;
    void* const* out_values;
    void* const* out_offsets;
    uint8_t* const* out_validity;
    uint64_t* value_bytes;
    uint32_t* written;
};

inline uint32_t out_kind(const Args& a, uint32_t o) { return a.kinds[a.plan[4 * o]]; }
inline bool sizes_only(const Args& a) { return !a.out_values && !a.out_offsets && !a.out_validity; }
inline uint64_t bitmap_bytes(uint64_t rows) { return (rows + 7) >> 3; }
// value bytes of a column that is no byte column
inline uint64_t plain_value_bytes(uint32_t kind, uint64_t rows) {
    return kind == OXH_COL_BOOL ? bitmap_bytes(rows) : rows * cols::width_of(kind);
}

// "" when the arguments are well formed, else what is wrong with them (the order is the header's).
// host: the offsets can be read and are checked; else the outputs are device memory and the bit-packed
// ones must be 8-byte aligned.
inline std::string argument_error(const Args& a, bool host) {
    if (!a.kinds || !a.values || !a.offsets || !a.validity || !a.bit_offsets || !a.src_rows || !a.plan)
        return "kinds, values, offsets, validity, bit_offsets, src_rows or plan is NULL";
    if (a.nsrc == 0 || a.nout == 0) return "nsrc or nout is 0";
    for (uint32_t c = 0; c < a.nsrc; ++c)
        if (!cols::known_kind(a.kinds[c])) return "column " + std::to_string(c) + " has unknown kind " + std::to_string(a.kinds[c]);
    for (uint32_t o = 0; o < a.nout; ++o) {
        const uint32_t *p = a.plan + 4 * o, b = p[2];
        const std::string out = "output column " + std::to_string(o);
        if (p[0] >= a.nsrc || (b != OXH_TAKE_NO_COLUMN && b >= a.nsrc)) return out + " names a source column that is not there";
        if (p[1] > 1 || (b != OXH_TAKE_NO_COLUMN && p[3] > 1)) return out + " names an index array other than 0 and 1";
    }
    for (uint32_t o = 0; o < a.nout; ++o) {
        const uint32_t* p = a.plan + 4 * o;
        if (p[2] != OXH_TAKE_NO_COLUMN && a.kinds[p[0]] != a.kinds[p[2]])
            return "output column " + std::to_string(o) + ": the fallback column's kind differs";
    }
    if (a.nout_rows > kMaxRows) return "more than 2^32 - 2 output rows";
    for (uint32_t c = 0; c < a.nsrc; ++c)
        if (a.src_rows[c] > kMaxRows) return "column " + std::to_string(c) + " has more than 2^32 - 2 rows";
    if (!a.value_bytes || !a.written) return "value_bytes or written is NULL";
    for (uint32_t c = 0; c < a.nsrc; ++c)
        if (a.src_rows[c] && cols::is_bytes(a.kinds[c]) && !a.offsets[c])
            return "column " + std::to_string(c) + " is a byte column without offsets";
    for (uint32_t c = 0; c < a.nsrc; ++c) {
        if (!a.src_rows[c]) continue;
        const std::string what = cols::column_error("column " + std::to_string(c), a.kinds[c], a.values[c], a.offsets[c], a.src_rows[c], host);
        if (!what.empty()) return what;
    }
    if (sizes_only(a)) return "";
    if (!a.out_values || !a.out_offsets || !a.out_validity) return "some of out_values, out_offsets, out_validity are NULL and some are not";
    if (!a.value_capacity) return "outputs without value_capacity";
    for (uint32_t o = 0; o < a.nout; ++o) {
        const uint32_t kind = out_kind(a, o);
        const std::string out = "output column " + std::to_string(o);
        if (cols::is_bytes(kind) && !a.out_offsets[o]) return out + " is a byte column without out_offsets";
        if (!a.nout_rows) continue;
        if (!a.out_validity[o]) return out + " has no out_validity";
        if (!cols::is_bytes(kind) && !a.out_values[o]) return out + " has no out_values";
        if (cols::is_bytes(kind) && a.value_capacity[o] && !a.out_values[o]) return out + " has value_capacity but no out_values";
        if (!host && (((uintptr_t)a.out_validity[o] & 7) || (kind == OXH_COL_BOOL && ((uintptr_t)a.out_values[o] & 7))))
            return out + ": a bit-packed output is not 8-byte aligned";
    }
    return "";
}

// The host form's second device block: for every output column its validity, values and offsets, each piece
// 16-B aligned (so every bit-packed piece is 8-byte aligned). at[3 * o + {0, 1, 2}] = where they start;
// value_bytes[o] = the bytes of column o's values.
struct OutBlock {
    std::vector<uint64_t> at;
    uint64_t total = 0;
    OutBlock(const Args& a, const uint64_t* value_bytes) : at(3 * (size_t)a.nout, 0) {
        auto add = [&](uint64_t bytes) {
            const uint64_t here = total;
            total += (bytes + 15) & ~15ull;
            return here;
        };
        for (uint32_t o = 0; o < a.nout; ++o) {
            const uint32_t kind = out_kind(a, o);
            at[3 * o] = add(bitmap_bytes(a.nout_rows));
            at[3 * o + 1] = add(value_bytes[o]);
            at[3 * o + 2] = add(cols::is_bytes(kind) ? (a.nout_rows + 1) * cols::offset_width(kind) : 0);
        }
    }
};

}  // namespace oxh::take
