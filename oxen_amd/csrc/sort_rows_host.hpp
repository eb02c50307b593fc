// oxen_amd/csrc/sort_rows_host.hpp -- the host-only pieces of oxh_sort_rows_* (sort_rows.hip): what both
// forms check before they need a device and the host form's staging plan (columns.hpp's, one device block
// for the permutation and the key columns). Plain C++ with
// no HIP in it, so that a stand-alone program can call it (tests/native/sort_rows_host_test.cpp, which is
// also what a sanitizer build runs).
#pragma once

#include "columns.hpp"
#include "sort_keys.hpp"

namespace oxh::sortrows {

constexpr uint64_t kMaxRows = 0xFFFFFFFEull;  // row indices are u32, and usable as the take's idx0

struct Args {
    uint64_t nrows;
    uint32_t nkeys;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint32_t* orders;
    uint32_t* perm;
    uint64_t* stats3;
};

inline bool known_order(uint32_t order) { return order == OXH_SORT_SIGNED || order == OXH_SORT_UNSIGNED || order == OXH_SORT_FLOAT; }

// "" when the arguments are well formed, else what is wrong with them (the order is the header's).
// host: the offsets can be read and are checked.
inline std::string argument_error(const Args& a, bool host) {
    if (!a.kinds || !a.values || !a.offsets || !a.validity || !a.bit_offsets || !a.orders)
        return "kinds, values, offsets, validity, bit_offsets or orders is NULL";
    if (a.nkeys == 0) return "nkeys is 0";
    for (uint32_t c = 0; c < a.nkeys; ++c) {
        const std::string col = "key column " + std::to_string(c);
        if (!cols::known_kind(a.kinds[c])) return col + " has unknown kind " + std::to_string(a.kinds[c]);
        if (cols::width_of(a.kinds[c]) && !known_order(a.orders[c])) return col + " has unknown order class " + std::to_string(a.orders[c]);
    }
    for (uint32_t c = 0; c < a.nkeys; ++c)
        if (a.kinds[c] == OXH_COL_FIXED1 && a.orders[c] == OXH_SORT_FLOAT)
            return "key column " + std::to_string(c) + ": OXH_SORT_FLOAT needs a width of 4 or 8";
    if (a.nrows > kMaxRows) return "more than 2^32 - 2 rows";
    if (a.nrows) {
        for (uint32_t c = 0; c < a.nkeys; ++c) {
            const std::string what = cols::column_error("key column " + std::to_string(c), a.kinds[c], a.values[c], a.offsets[c], a.nrows, host);
            if (!what.empty()) return what;
        }
        if (!a.perm) return "perm is NULL";
    }
    if (!a.stats3) return "stats3 is NULL";
    return "";
}

// The host form's device block: the permutation (nrows u32) at its front, then every key column as
// columns.hpp stages it.
struct HostPlan {
    cols::Staging staging;
    std::vector<cols::Staged> staged;
    explicit HostPlan(const Args& a) : staged(a.nkeys) {
        staging.total = (a.nrows * 4 + 15) & ~15ull;
        for (uint32_t c = 0; c < a.nkeys; ++c)
            staged[c] = staging.add_column(a.kinds[c], a.values[c], a.offsets[c], a.validity[c], a.bit_offsets[2 * c],
                                           a.bit_offsets[2 * c + 1], a.nrows);
    }
};

}  // namespace oxh::sortrows
