// oxen_amd/csrc/group_rows_host.hpp -- the host-only pieces of oxh_group_rows_* (group_rows.hip): what both
// forms check before they need a device, the device memory a call leases, and the host form's staging plan
// (columns.hpp's, one device block for the four output arrays and the key columns). Plain C++ with no HIP in
// it, so that a stand-alone program can call it (tests/native/group_rows_host_test.cpp, which is also what a
// sanitizer build runs).
#pragma once

#include "columns.hpp"
#include "sort_rows_host.hpp"

namespace oxh::grouprows {

constexpr uint64_t kMaxRows = sortrows::kMaxRows;  // row indices are u32, and usable as the take's idx0

struct Args {
    uint64_t nrows;
    uint32_t nkeys;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint32_t* orders;
    uint32_t *group, *count, *first_idx, *first_count;  // each may be NULL
    uint64_t* stats4;
};

// "" when the arguments are well formed, else what is wrong with them: the sort's list in the sort's order
// (sort_rows_host.hpp) -- the key columns are described in the same way -- but for the outputs: every array
// may be NULL, stats4 may not.
inline std::string argument_error(const Args& a, bool host) {
    uint32_t some_perm = 0;
    uint64_t some_stats[3];
    const sortrows::Args s{a.nrows, a.nkeys, a.kinds, a.values, a.offsets, a.validity, a.bit_offsets, a.orders, &some_perm, some_stats};
    const std::string what = sortrows::argument_error(s, host);
    if (!what.empty()) return what;
    if (!a.stats4) return "stats4 is NULL";
    return "";
}

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
inline uint64_t scan_tiles_of(uint64_t n) { return (n + 2047) / 2048; }  // keyed_diff.hip's scan_tiles (checked where the lease is made)

// The row-shaped device memory of one call, leased from scratch.hpp (offsets into the lease; the long rows'
// scratch of the key images follows at `total`): the key digests (16 B per row), each row's id from the index
// (8), the groups' sizes (4), the first-occurrence flags (4) and their scan (8): 40 B per row.
struct Lease {
    uint64_t digests, first, count_of, flag, flag_scan, sums, total;
    explicit Lease(uint64_t n) {
        uint64_t at = 0;
        auto carve = [&](uint64_t bytes) {
            const uint64_t here = at;
            at += align256(bytes);
            return here;
        };
        digests = carve(n * 16);
        first = carve(n * 8);
        count_of = carve(n * 4);
        flag = carve(n * 4);
        flag_scan = carve(n * 8);
        sums = carve((scan_tiles_of(n) + 1) * 8);
        total = at;
    }
};

// The host form's device block: the four output arrays (nrows u32 each, 16-B aligned) at its front, then
// every key column as columns.hpp stages it.
struct HostPlan {
    cols::Staging staging;
    std::vector<cols::Staged> staged;
    uint64_t out_bytes;  // of one output array
    explicit HostPlan(const Args& a) : staged(a.nkeys), out_bytes((a.nrows * 4 + 15) & ~15ull) {
        staging.total = 4 * out_bytes;
        for (uint32_t c = 0; c < a.nkeys; ++c)
            staged[c] = staging.add_column(a.kinds[c], a.values[c], a.offsets[c], a.validity[c], a.bit_offsets[2 * c],
                                           a.bit_offsets[2 * c + 1], a.nrows);
    }
};

}  // namespace oxh::grouprows
