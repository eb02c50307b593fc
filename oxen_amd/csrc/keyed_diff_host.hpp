// oxen_amd/csrc/keyed_diff_host.hpp -- the host-only pieces of oxh_keyed_diff_* (keyed_diff.hip): what both
// forms check before they need a device, and the host form's ordering of a left row's pairs. Plain C++
// with no HIP in it, so that a stand-alone program can call it (tests/native/keyed_diff_host_test.cpp,
// which is also what a sanitizer build runs).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace oxh::keyed {

constexpr uint64_t kMaxRows = 0xFFFFFFFEull;   // row indices are u32 and 0xFFFFFFFF is "absent"
constexpr uint32_t kNone = 0xFFFFFFFFu;        // OXH_KEYED_DIFF_NONE
constexpr uint32_t kKnownFlags = 1;            // OXH_KEYED_DIFF_KEEP_UNCHANGED

// Two tables of n (lo, hi) rows that share some of their bytes without being one table.
inline bool partly_overlap(const uint64_t* a, const uint64_t* b, uint64_t n) {
    if (!a || !b || a == b || n == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)(n * 16);
    return x < y ? y - x < bytes : x - y < bytes;
}

// NULL when the arguments are well formed, else what is wrong with them (the order is the header's).
inline const char* argument_error(const uint64_t* left_keys, uint64_t nleft, const uint64_t* right_keys, uint64_t nright,
                                  const uint64_t* left_targets, const uint64_t* right_targets, const uint64_t* bit_offsets2,
                                  uint32_t flags, uint64_t capacity, const uint32_t* left_idx, const uint32_t* right_idx,
                                  const uint8_t* status, const uint64_t* counts8) {
    if (!counts8 || !bit_offsets2) return "counts8 or bit_offsets2 is NULL";
    if (nleft > kMaxRows || nright > kMaxRows) return "more than 2^32 - 2 rows on a side";
    if ((nleft && !left_keys) || (nright && !right_keys)) return "a key table is NULL";
    if (partly_overlap(left_keys, left_targets, nleft) || partly_overlap(right_keys, right_targets, nright))
        return "a target table overlaps its side's key table without being the same table";
    if (capacity && (!left_idx || !right_idx || !status)) return "capacity > 0 with a NULL output array";
    if (flags & ~kKnownFlags) return "unknown flag";
    return nullptr;
}

// The pairs of one call in the canonical order but for the right rows of one left row, which the device
// writes as its bucket was filled: sort them ascending inside every run of equal left_idx (statuses move
// with their rows). The right-only rows at the end (left_idx == kNone) are ascending already.
inline void sort_runs(uint32_t* left_idx, uint32_t* right_idx, uint8_t* status, uint64_t n) {
    std::vector<std::pair<uint32_t, uint8_t>> run;
    for (uint64_t i = 0; i < n;) {
        uint64_t j = i + 1;
        while (j < n && left_idx[j] == left_idx[i]) ++j;
        if (j - i > 1 && left_idx[i] != kNone) {
            run.clear();
            for (uint64_t k = i; k < j; ++k) run.emplace_back(right_idx[k], status[k]);
            std::sort(run.begin(), run.end());
            for (uint64_t k = i; k < j; ++k) right_idx[k] = run[k - i].first, status[k] = run[k - i].second;
        }
        i = j;
    }
}

}  // namespace oxh::keyed
