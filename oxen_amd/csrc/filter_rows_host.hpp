// oxen_amd/csrc/filter_rows_host.hpp -- the host-only pieces of oxh_filter_rows_* (filter_rows.hip): what both
// forms check before they need a device, the device memory a call leases, and the host form's staging plan
// (columns.hpp's, one device block for idx, the mask and only the columns the terms name). Plain C++ with no
// HIP in it, so that a stand-alone program can call it (tests/native/filter_rows_host_test.cpp, which is also
// what a sanitizer build runs).
#pragma once

#include "columns.hpp"
#include "filter_terms.hpp"
#include "sort_rows_host.hpp"

namespace oxh::filterrows {

constexpr uint64_t kMaxRows = sortrows::kMaxRows;  // row indices are u32, and usable as the take's idx0

struct Args {
    uint64_t nrows;
    uint32_t ncols;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint32_t* orders;
    uint32_t nterms;
    const uint32_t* term_col;
    const uint32_t* term_op;
    const uint64_t* term_word;
    const uint8_t* lit_bytes;
    const uint64_t* lit_offsets;
    const uint32_t* logical;
    uint32_t* idx;    // may be NULL
    uint64_t* mask;   // may be NULL
    uint64_t* stats2;
};

// "" when the arguments are well formed, else what is wrong with them, in the header's order: the sort's list
// in the sort's order (sort_rows_host.hpp) over the ncols columns -- they are described in the same way -- then
// the terms, then stats2.
inline std::string argument_error(const Args& a, bool host) {
    uint32_t some_perm = 0;
    uint64_t some_stats[3];
    const sortrows::Args s{a.nrows, a.ncols, a.kinds, a.values, a.offsets, a.validity, a.bit_offsets, a.orders, &some_perm, some_stats};
    const std::string what = sortrows::argument_error(s, host);
    if (!what.empty()) return what == "nkeys is 0" ? "ncols is 0" : what;
    if (a.nterms == 0) return "nterms is 0";
    if (a.nterms > OXH_FILTER_MAX_TERMS) return "more than OXH_FILTER_MAX_TERMS (" + std::to_string(OXH_FILTER_MAX_TERMS) + ") terms";
    if (!a.term_col || !a.term_op || !a.term_word || !a.lit_offsets) return "term_col, term_op, term_word or lit_offsets is NULL";
    if (a.nterms > 1 && !a.logical) return "logical is NULL with more than one term";
    for (uint32_t t = 0; t < a.nterms; ++t)
        if (a.term_col[t] >= a.ncols) return "term " + std::to_string(t) + " names column " + std::to_string(a.term_col[t]) + " of " + std::to_string(a.ncols);
    for (uint32_t t = 0; t < a.nterms; ++t)
        if (!filterterms::known_op(a.term_op[t])) return "term " + std::to_string(t) + " has unknown operator " + std::to_string(a.term_op[t]);
    for (uint32_t t = 0; t + 1 < a.nterms; ++t)
        if (!filterterms::known_logical(a.logical[t])) return "unknown logical operator " + std::to_string(a.logical[t]) + " after term " + std::to_string(t);
    for (uint32_t t = 0; t < a.nterms; ++t)
        if (a.kinds[a.term_col[t]] == OXH_COL_BOOL && a.term_word[t] > 1) return "term " + std::to_string(t) + ": a boolean literal is 0 or 1";
    for (uint32_t t = 0; t < a.nterms; ++t)
        if (a.lit_offsets[t + 1] < a.lit_offsets[t]) return "lit_offsets decrease at term " + std::to_string(t);
    if (a.lit_offsets[a.nterms] > OXH_FILTER_MAX_LITERAL_BYTES)
        return "more than OXH_FILTER_MAX_LITERAL_BYTES (" + std::to_string(OXH_FILTER_MAX_LITERAL_BYTES) + ") bytes of literals";
    if (!a.lit_bytes && a.lit_offsets[a.nterms] > a.lit_offsets[0]) return "lit_bytes is NULL with a literal that is not empty";
    if (!a.stats2) return "stats2 is NULL";
    return "";
}

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
inline uint64_t blocks_of(uint64_t n) { return (n + 63) / 64; }               // 64-row blocks: one mask word each
inline uint64_t scan_tiles_of(uint64_t n) { return (n + 2047) / 2048; }       // keyed_diff.hip's scan_tiles (checked where the lease is made)

// The literals as the kernel gets them: every byte term's literal at an 8-byte aligned place of one block of
// at most kLitBlock bytes, so that eight bytes of it are one aligned read.
constexpr uint64_t kLitBlock = OXH_FILTER_MAX_LITERAL_BYTES + 8 * OXH_FILTER_MAX_TERMS;
constexpr uint64_t kCtrlBytes = 256;  // the control words of a call

// The device memory of one call, leased from scratch.hpp (offsets into the lease): the control words and the
// literal block (4.4 KiB together), and for a call that wants idx, per 64-row block, the selected rows of the
// block (4 B) and their scan (8 B) -- 12 B per 64 rows -- and, where the caller takes no mask, the mask words
// the emit reads (8 B).
struct Lease {
    uint64_t ctrl, lits, counts, bases, sums, mask, total;
    Lease(uint64_t n, bool want_idx, bool own_mask) {
        const uint64_t blocks = want_idx ? blocks_of(n) : 0;
        uint64_t at = 0;
        auto carve = [&](uint64_t bytes) {
            const uint64_t here = at;
            at += align256(bytes);
            return here;
        };
        ctrl = carve(kCtrlBytes);
        lits = carve(kLitBlock);
        counts = carve(blocks * 4);
        bases = carve(blocks * 8);
        sums = carve(want_idx ? (scan_tiles_of(blocks) + 1) * 8 : 0);
        mask = want_idx && own_mask ? carve(blocks * 8) : at;
        total = at;
    }
};

struct Literals {
    std::vector<uint8_t> bytes;                         // a multiple of 8
    uint32_t at[OXH_FILTER_MAX_TERMS] = {}, len[OXH_FILTER_MAX_TERMS] = {};
    explicit Literals(const Args& a) {
        for (uint32_t t = 0; t < a.nterms; ++t) {
            if (!cols::is_bytes(a.kinds[a.term_col[t]])) continue;
            at[t] = (uint32_t)bytes.size();
            len[t] = (uint32_t)(a.lit_offsets[t + 1] - a.lit_offsets[t]);
            if (len[t]) bytes.insert(bytes.end(), a.lit_bytes + a.lit_offsets[t], a.lit_bytes + a.lit_offsets[t + 1]);
            bytes.resize((bytes.size() + 7) & ~(size_t)7, 0);
        }
    }
};

// bit t - 1: the logical operator between the fold so far and term t is ||
inline uint32_t or_bits_of(const Args& a) {
    uint32_t bits = 0;
    for (uint32_t t = 0; t + 1 < a.nterms; ++t)
        if (a.logical[t] == OXH_FILTER_OR) bits |= 1u << t;
    return bits;
}

// The host form's device block: idx (nrows u32) and the mask (a word per 64 rows) at its front, 16-B aligned
// each and there whether or not the caller takes them, then every column a term names -- once, however many
// terms name it -- as columns.hpp stages it. staged_of[c]: column c's entry in `staged`, -1 for a column no
// term names.
struct HostPlan {
    cols::Staging staging;
    std::vector<cols::Staged> staged;
    std::vector<int32_t> staged_of;
    uint64_t idx_bytes, mask_bytes;
    explicit HostPlan(const Args& a)
        : staged_of(a.ncols, -1), idx_bytes((a.nrows * 4 + 15) & ~15ull), mask_bytes((blocks_of(a.nrows) * 8 + 15) & ~15ull) {
        staging.total = idx_bytes + mask_bytes;
        for (uint32_t t = 0; t < a.nterms; ++t) {
            const uint32_t c = a.term_col[t];
            if (staged_of[c] >= 0) continue;
            staged_of[c] = (int32_t)staged.size();
            staged.push_back(staging.add_column(a.kinds[c], a.values[c], a.offsets[c], a.validity[c], a.bit_offsets[2 * c],
                                                a.bit_offsets[2 * c + 1], a.nrows));
        }
    }
};

}  // namespace oxh::filterrows
