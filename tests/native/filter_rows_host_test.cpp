// tests/native/filter_rows_host_test.cpp -- the terms of the row filter and the host-only pieces of
// oxh_filter_rows_* in a program of their own: filter_terms.hpp -- the code the kernel runs -- over every
// operator and compare outcome, the nine Kleene pairs of && and ||, the fold's left association, compare_bytes
// at the lengths around its 8-byte steps, the float canonical cases; and filter_rows_host.hpp: the argument
// checks in the header's order, the lease's layout, the literal block and the host form's staging plan. No HIP
// and no library: g++ -std=c++17 (add -fsanitize=address,undefined for a sanitizer run). Prints "ok" and exits
// 0, or says what failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../oxen_amd/csrc/filter_rows_host.hpp"

using namespace oxh;
namespace ft = oxh::filterterms;

static int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static bool says(const std::string& got, const char* part) { return got.find(part) != std::string::npos; }

static void operators() {
    EXPECT(OXH_FILTER_EQ == 0 && OXH_FILTER_NE == 1 && OXH_FILTER_LT == 2 && OXH_FILTER_LE == 3 && OXH_FILTER_GT == 4 && OXH_FILTER_GE == 5);
    EXPECT(OXH_FILTER_AND == 0 && OXH_FILTER_OR == 1 && OXH_FILTER_MAX_TERMS == 16 && OXH_FILTER_MAX_LITERAL_BYTES == 4096);
    // every operator x every compare outcome: {cmp < 0, cmp == 0, cmp > 0}
    const bool want[6][3] = {{false, true, false}, {true, false, true}, {true, false, false},
                             {true, true, false},  {false, false, true}, {false, true, true}};
    for (uint32_t op = 0; op < 6; ++op)
        for (int cmp = -1; cmp <= 1; ++cmp) {
            EXPECT(ft::holds(op, cmp) == want[op][cmp + 1]);
            EXPECT(ft::term_result(op, cmp) == (want[op][cmp + 1] ? ft::kTrue : ft::kFalse));
        }
    for (uint32_t op = 0; op < 8; ++op) EXPECT(ft::known_op(op) == (op < 6));
    EXPECT(ft::known_logical(0) && ft::known_logical(1) && !ft::known_logical(2));
}

static void kleene() {
    const uint32_t F = ft::kFalse, T = ft::kTrue, N = ft::kNull;
    const uint32_t v[3] = {F, T, N};
    const uint32_t want_and[3][3] = {{F, F, F}, {F, T, N}, {F, N, N}};
    const uint32_t want_or[3][3] = {{F, T, N}, {T, T, T}, {N, T, N}};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            EXPECT(ft::and3(v[a], v[b]) == want_and[a][b]);
            EXPECT(ft::or3(v[a], v[b]) == want_or[a][b]);
        }
    // the fold is left to right with no precedence: a || b && c is (a || b) && c
    {
        const uint32_t r[3] = {T, F, F};   // T || F && F: (T || F) && F = F, where precedence would give T
        EXPECT(ft::fold(r, 3, 0b01) == F);
        const uint32_t s[3] = {F, F, T};   // F && F || T: (F && F) || T = T either way
        EXPECT(ft::fold(s, 3, 0b10) == T);
        const uint32_t u[3] = {T, T, F};   // T || T && F = F, precedence: T
        EXPECT(ft::fold(u, 3, 0b01) == F);
        const uint32_t w[4] = {N, T, F, T};  // ((N || T) && F) || T = T; ((N && T) || F) && T = N
        EXPECT(ft::fold(w, 4, 0b101) == T && ft::fold(w, 4, 0b010) == N);
        EXPECT(ft::fold(w, 1, 0) == N && ft::fold(w + 1, 1, 0xFFFF) == T);
    }
    uint32_t all[16];
    for (uint32_t& x : all) x = T;
    EXPECT(ft::fold(all, 16, 0) == T);
    all[15] = F;
    EXPECT(ft::fold(all, 16, 0) == F && ft::fold(all, 16, 1u << 14) == T);
    EXPECT(ft::fold_step(N, F, 1, 0) == F && ft::fold_step(N, T, 1, 1) == T && ft::fold_step(N, F, 1, 1) == N);
}

static int cb(const std::string& cell, const std::string& lit) {
    // copies of the exact lengths, so that a sanitizer build sees any read past either span
    std::vector<uint8_t> c(cell.begin(), cell.end()), l(lit.begin(), lit.end());
    return ft::compare_bytes(c.data(), c.size(), l.data(), l.size());
}

static void bytes() {
    using S = std::string;
    EXPECT(cb("", "") == 0 && cb("", "a") == -1 && cb("a", "") == 1);
    EXPECT(cb("ab", "abc") == -1 && cb("abc", "ab") == 1 && cb("abc", "abc") == 0);          // a proper prefix first
    EXPECT(cb(S("a\0", 2), "a") == 1 && cb("a", S("a\0", 2)) == -1 && cb(S("a\0", 2), S("a\0", 2)) == 0);
    EXPECT(cb(S("a\0b", 3), S("a\0c", 3)) == -1 && cb(S("\0", 1), "") == 1);
    EXPECT(cb("\xff", "a") == 1 && cb("a", "\xff") == -1 && cb("\x80", "\x7f") == 1);     // unsigned bytes
    const S base = "0123456789abcdefXYZ";
    for (const size_t n : {7u, 8u, 9u, 16u, 17u}) {
        const S lit = base.substr(0, n);
        EXPECT(cb(lit, lit) == 0);
        EXPECT(cb(lit.substr(0, n - 1), lit) == -1 && cb(lit + "!", lit) == 1);
        for (size_t at = 0; at < n; ++at) {   // one byte differs, at every place: the first difference decides
            S lo = lit, hi = lit;
            lo[at] = (char)(lit[at] - 1), hi[at] = (char)(lit[at] + 1);
            EXPECT(cb(lo, lit) == -1 && cb(hi, lit) == 1);
            S both = lit;   // a lower byte first, a higher one behind it
            both[at] = (char)(lit[at] - 1);
            if (at + 1 < n) both[at + 1] = (char)0xFF;
            EXPECT(cb(both, lit) == -1);
            EXPECT(cb(lo + "zzzzzzzzz", lit) == -1 && cb(hi, lit + "zzzzzzzzz") == 1);
        }
    }
    // inside one 8-byte step the bytes compare big-endian: the first differing byte, not the last
    EXPECT(cb("a\xff\xff\xff\xff\xff\xff\xff", "b\0\0\0\0\0\0\0") == -1);
    // == and != of another length are decided without a read: the pointers are never followed
    const uint8_t* nowhere = nullptr;
    EXPECT(ft::compare_bytes_for(OXH_FILTER_EQ, nowhere, 5, nowhere, 6) != 0 && ft::compare_bytes_for(OXH_FILTER_NE, nowhere, 300, nowhere, 0) != 0);
    EXPECT(ft::compare_bytes(nowhere, 0, nowhere, 0) == 0 && ft::compare_bytes(nowhere, 0, (const uint8_t*)"a", 1) == -1);
    const uint8_t abc[3] = {'a', 'b', 'c'}, abd[3] = {'a', 'b', 'd'};
    for (uint32_t op = 0; op < 6; ++op) {
        EXPECT(ft::compare_bytes_for(op, abc, 3, abd, 3) == -1 && ft::compare_bytes_for(op, abc, 3, abc, 3) == 0);
        if (op >= OXH_FILTER_LT) EXPECT(ft::compare_bytes_for(op, abc, 2, abc, 3) == -1 && ft::compare_bytes_for(op, abd, 3, abc, 2) == 1);
    }
}

static uint64_t f64(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
static uint64_t f32(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

static void fixed() {
    // Int8 0xFF: -1 signed, 255 unsigned
    EXPECT(ft::compare_fixed(OXH_SORT_SIGNED, 1, 0xFF, 0) == -1 && ft::compare_fixed(OXH_SORT_UNSIGNED, 1, 0xFF, 0) == 1);
    EXPECT(ft::compare_fixed(OXH_SORT_SIGNED, 1, 0x80, 0x7F) == -1 && ft::compare_fixed(OXH_SORT_SIGNED, 1, 0xFF, 0xFF) == 0);
    EXPECT(ft::compare_fixed(OXH_SORT_SIGNED, 4, 0xFFFFFFFFull, 1) == -1 && ft::compare_fixed(OXH_SORT_UNSIGNED, 4, 0xFFFFFFFFull, 1) == 1);
    EXPECT(ft::compare_fixed(OXH_SORT_SIGNED, 8, ~0ull, 0) == -1 && ft::compare_fixed(OXH_SORT_UNSIGNED, 8, ~0ull, 0) == 1);
    EXPECT(ft::compare_fixed(OXH_SORT_SIGNED, 8, (uint64_t)INT64_MIN, (uint64_t)INT64_MAX) == -1);
    // the literal's bytes above the width are ignored
    EXPECT(ft::compare_fixed(OXH_SORT_SIGNED, 1, 5, 0xABCD05) == 0 && ft::compare_fixed(OXH_SORT_UNSIGNED, 4, 7, 0x100000007ull) == 0);
    EXPECT(ft::low_bytes(~0ull, 1) == 0xFF && ft::low_bytes(~0ull, 4) == 0xFFFFFFFFull && ft::low_bytes(~0ull, 8) == ~0ull);
    // floats: numeric, -0.0 == +0.0, every NaN equal to every NaN and above +inf
    const double inf = INFINITY;
    EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(-0.0), f64(0.0)) == 0 && ft::compare_fixed(OXH_SORT_FLOAT, 4, f32(-0.0f), f32(0.0f)) == 0);
    EXPECT(ft::compare_fixed(OXH_SORT_UNSIGNED, 8, f64(-0.0), f64(0.0)) == 1);
    EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(-1.5), f64(0.5)) == -1 && ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(-1.5), f64(-2.5)) == 1);
    EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(-inf), f64(-1e308)) == -1 && ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(inf), f64(1e308)) == 1);
    EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(5e-324), f64(0.0)) == 1 && ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(-5e-324), f64(-0.0)) == -1);
    const uint64_t nans64[4] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, 0xFFF5A5A5A5A5A5A5ull};
    const uint64_t nans32[4] = {0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFFA55AA5u};
    for (const uint64_t a : nans64) {
        for (const uint64_t b : nans64) EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 8, a, b) == 0);
        EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 8, a, f64(inf)) == 1 && ft::compare_fixed(OXH_SORT_FLOAT, 8, f64(-inf), a) == -1);
    }
    for (const uint64_t a : nans32) {
        for (const uint64_t b : nans32) EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 4, a, b) == 0);
        EXPECT(ft::compare_fixed(OXH_SORT_FLOAT, 4, a, f32(INFINITY)) == 1 && ft::compare_fixed(OXH_SORT_FLOAT, 4, f32(1.0f), a) == -1);
    }
    EXPECT(ft::compare_words(0, 1) == -1 && ft::compare_words(1, 1) == 0 && ft::compare_words(~0ull, 1) == 1);  // booleans: false < true
}

// Three columns of 3 rows: Int32, Boolean, BYTES32; three terms: c0 > 1 && c1 == true || c2 != "ab".
struct Call {
    int32_t ints[3] = {1, -2, 3};
    uint8_t bools[1] = {0b101};
    char text[7] = "abcdef";
    int32_t off[4] = {1, 3, 3, 6};
    uint8_t valid[1] = {0b011};
    uint32_t kinds[3] = {OXH_COL_FIXED4, OXH_COL_BOOL, OXH_COL_BYTES32};
    const void* values[3] = {ints, bools, text};
    const void* offsets[3] = {nullptr, nullptr, off};
    const uint8_t* validity[3] = {nullptr, valid, nullptr};
    uint64_t bits[6] = {0, 0, 0, 0, 0, 0};
    uint32_t orders[3] = {OXH_SORT_SIGNED, 0, 0};
    uint32_t term_col[3] = {0, 1, 2};
    uint32_t term_op[3] = {OXH_FILTER_GT, OXH_FILTER_EQ, OXH_FILTER_NE};
    uint64_t term_word[3] = {1, 1, 0};
    uint8_t lit[2] = {'a', 'b'};
    uint64_t lit_off[4] = {0, 0, 0, 2};
    uint32_t logical[2] = {OXH_FILTER_AND, OXH_FILTER_OR};
    uint32_t idx[3] = {9, 9, 9};
    uint64_t mask[1] = {9};
    uint64_t stats[2] = {7, 7};
    filterrows::Args a{3, 3, kinds, values, offsets, validity, bits, orders, 3, term_col, term_op, term_word, lit, lit_off, logical, idx, mask, stats};
};

static void arguments() {
    for (const bool host : {true, false}) {
        auto err = [&](const Call& d) { return filterrows::argument_error(d.a, host); };
        Call c;
        EXPECT(err(c).empty());
        // 1. the sort's list
        { Call d; d.a.kinds = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.values = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.offsets = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.validity = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.bit_offsets = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.orders = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.ncols = 0; EXPECT(says(err(d), "ncols is 0")); }
        { Call d; d.kinds[1] = 33; EXPECT(says(err(d), "unknown kind")); }
        { Call d; d.orders[0] = 3; EXPECT(says(err(d), "unknown order class")); }
        { Call d; d.orders[1] = 77, d.orders[2] = 99; EXPECT(err(d).empty()); }  // ignored there
        { Call d; d.kinds[0] = OXH_COL_FIXED1, d.orders[0] = OXH_SORT_FLOAT; EXPECT(says(err(d), "width of 4 or 8")); }
        { Call d; d.a.nrows = 0xFFFFFFFFull; EXPECT(says(err(d), "2^32 - 2")); }
        { Call d; d.offsets[2] = nullptr; EXPECT(says(err(d), "without offsets")); }
        { Call d; d.values[0] = nullptr; EXPECT(says(err(d), "has no values")); }
        // 2. .. 9. the terms
        { Call d; d.a.nterms = 0; EXPECT(says(err(d), "nterms is 0")); }
        { Call d; d.a.nterms = 17; EXPECT(says(err(d), "OXH_FILTER_MAX_TERMS")); }
        { Call d; d.a.term_col = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.term_op = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.term_word = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.lit_offsets = nullptr; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.a.logical = nullptr; EXPECT(says(err(d), "logical is NULL")); }
        { Call d; d.a.logical = nullptr, d.a.nterms = 1; EXPECT(err(d).empty()); }
        { Call d; d.term_col[1] = 3; EXPECT(says(err(d), "names column 3")); }
        { Call d; d.term_op[2] = 6; EXPECT(says(err(d), "unknown operator")); }
        { Call d; d.logical[1] = 2; EXPECT(says(err(d), "unknown logical operator")); }
        { Call d; d.logical[1] = 2, d.a.nterms = 2; EXPECT(err(d).empty()); }   // only nterms - 1 entries are read
        { Call d; d.term_word[1] = 2; EXPECT(says(err(d), "boolean literal")); }
        { Call d; d.term_word[0] = ~0ull; EXPECT(err(d).empty()); }              // a fixed-width literal is any word
        { Call d; d.lit_off[1] = 1, d.lit_off[2] = 0; EXPECT(says(err(d), "lit_offsets decrease")); }
        { Call d; d.lit_off[3] = 4097; EXPECT(says(err(d), "OXH_FILTER_MAX_LITERAL_BYTES")); }
        { Call d; d.lit_off[3] = 4096; EXPECT(err(d).empty()); }                 // looked at by nobody here
        { Call d; d.a.lit_bytes = nullptr; EXPECT(says(err(d), "lit_bytes is NULL")); }
        { Call d; d.a.lit_bytes = nullptr, d.lit_off[3] = 0; EXPECT(err(d).empty()); }   // the literal ""
        { Call d; d.a.stats2 = nullptr; EXPECT(says(err(d), "stats2 is NULL")); }
        // both outputs may be NULL, alone or together
        for (int m = 0; m < 4; ++m) {
            Call d;
            if (m & 1) d.a.idx = nullptr;
            if (m & 2) d.a.mask = nullptr;
            EXPECT(err(d).empty());
        }
        {   // the offsets are read only where they are host memory
            Call d;
            d.off[2] = 2;
            EXPECT(host ? says(err(d), "decrease") : err(d).empty());
            d.off[2] = 3, d.off[0] = -1;
            EXPECT(host ? says(err(d), "negative") : err(d).empty());
        }
        // the order of the checks
        { Call d; d.kinds[1] = 33, d.a.nterms = 0; EXPECT(says(err(d), "unknown kind")); }
        { Call d; d.values[0] = nullptr, d.a.nterms = 0; EXPECT(says(err(d), "has no values")); }
        { Call d; d.a.nterms = 0, d.a.term_col = nullptr; EXPECT(says(err(d), "nterms is 0")); }
        { Call d; d.a.nterms = 17, d.a.term_col = nullptr; EXPECT(says(err(d), "OXH_FILTER_MAX_TERMS")); }
        { Call d; d.a.term_op = nullptr, d.term_col[0] = 9; EXPECT(says(err(d), "is NULL")); }
        { Call d; d.term_col[0] = 9, d.term_op[0] = 9; EXPECT(says(err(d), "names column 9")); }
        { Call d; d.term_op[0] = 9, d.logical[0] = 9; EXPECT(says(err(d), "unknown operator")); }
        { Call d; d.logical[0] = 9, d.term_word[1] = 5; EXPECT(says(err(d), "unknown logical operator")); }
        { Call d; d.term_word[1] = 5, d.lit_off[3] = 9999; EXPECT(says(err(d), "boolean literal")); }
        { Call d; d.lit_off[0] = 3, d.a.lit_bytes = nullptr; EXPECT(says(err(d), "lit_offsets decrease")); }
        { Call d; d.a.lit_bytes = nullptr, d.a.stats2 = nullptr; EXPECT(says(err(d), "lit_bytes is NULL")); }
        // no rows: the arrays of the columns are not looked at, the terms and stats2 still are
        { Call d; d.a.nrows = 0, d.values[0] = nullptr, d.offsets[2] = nullptr; EXPECT(err(d).empty()); }
        { Call d; d.a.nrows = 0, d.a.nterms = 0; EXPECT(says(err(d), "nterms is 0")); }
        { Call d; d.a.nrows = 0, d.a.stats2 = nullptr; EXPECT(says(err(d), "stats2 is NULL")); }
        EXPECT(c.idx[0] == 9 && c.idx[2] == 9 && c.mask[0] == 9 && c.stats[0] == 7 && c.stats[1] == 7);
    }
}

static void lease() {
    for (const uint64_t n : {1ull, 63ull, 64ull, 65ull, 131072ull, 131073ull, 0xFFFFFFFEull}) {
        const uint64_t blocks = filterrows::blocks_of(n);
        EXPECT(blocks == (n + 63) / 64 && blocks * 64 >= n && (blocks - 1) * 64 < n);
        for (const bool own : {false, true}) {
            const filterrows::Lease at(n, true, own);
            // 256-B aligned pieces that do not overlap, in this order: the control words, the literal block, 12 B
            // per block, the scan's sums, 8 B of mask
            EXPECT(at.ctrl == 0 && at.lits >= filterrows::kCtrlBytes && at.counts >= at.lits + filterrows::kLitBlock);
            EXPECT(at.bases >= at.counts + blocks * 4 && at.sums >= at.bases + blocks * 8);
            EXPECT(at.mask >= at.sums + (filterrows::scan_tiles_of(blocks) + 1) * 8);
            EXPECT(at.total == (own ? at.mask + filterrows::align256(blocks * 8) : at.mask));
            for (const uint64_t x : {at.lits, at.counts, at.bases, at.sums, at.mask, at.total}) EXPECT(x % 256 == 0);
            EXPECT(at.total <= blocks * (own ? 20 : 12) + 4 * 256 + (blocks / 2048 + 2) * 8 + 256 + filterrows::kLitBlock + 256);
            // without idx: the control words and the literal block alone
            const filterrows::Lease none(n, false, own);
            EXPECT(none.ctrl == 0 && none.lits == at.lits && none.total == none.counts && none.total == at.counts && none.mask == none.total);
        }
    }
    EXPECT(filterrows::blocks_of(0) == 0 && filterrows::scan_tiles_of(2048) == 1 && filterrows::scan_tiles_of(2049) == 2);
    EXPECT(filterrows::kMaxRows == 0xFFFFFFFEull && filterrows::kCtrlBytes >= 3 * 8);
}

static void literals() {
    Call c;
    {
        const filterrows::Literals l(c.a);
        EXPECT(l.bytes.size() == 8 && l.at[2] == 0 && l.len[2] == 2 && l.bytes[0] == 'a' && l.bytes[1] == 'b' && l.bytes[2] == 0);
        EXPECT(l.len[0] == 0 && l.len[1] == 0);
        EXPECT(filterrows::or_bits_of(c.a) == 0b10);
    }
    {   // 16 byte terms of 256 B: the cap; every literal starts at a multiple of 8, the block holds them all
        std::vector<uint8_t> lit(4096);
        for (size_t b = 0; b < lit.size(); ++b) lit[b] = (uint8_t)(b * 7);
        uint32_t col[16], op[16], logical[15];
        uint64_t word[16] = {}, off[17];
        for (int t = 0; t < 16; ++t) col[t] = 2, op[t] = OXH_FILTER_EQ, off[t] = t * 256ull - (t ? t : 0);
        off[16] = 4096;                                   // lengths 255 .. 255, the last one longer: all odd places
        for (int t = 0; t < 15; ++t) logical[t] = t & 1;
        Call d;
        d.a.nterms = 16, d.a.term_col = col, d.a.term_op = op, d.a.term_word = word, d.a.lit_bytes = lit.data(), d.a.lit_offsets = off;
        d.a.logical = logical;
        EXPECT(filterrows::argument_error(d.a, true).empty());
        const filterrows::Literals l(d.a);
        EXPECT(l.bytes.size() % 8 == 0 && l.bytes.size() <= filterrows::kLitBlock);
        for (int t = 0; t < 16; ++t) {
            EXPECT(l.at[t] % 8 == 0 && l.len[t] == off[t + 1] - off[t] && l.at[t] + l.len[t] <= l.bytes.size());
            EXPECT(memcmp(l.bytes.data() + l.at[t], lit.data() + off[t], l.len[t]) == 0);
            if (t) EXPECT(l.at[t] >= l.at[t - 1] + l.len[t - 1]);
        }
        EXPECT(filterrows::or_bits_of(d.a) == 0b010101010101010);
    }
    EXPECT(filterrows::kLitBlock % 8 == 0 && filterrows::kLitBlock >= OXH_FILTER_MAX_LITERAL_BYTES + 7 * OXH_FILTER_MAX_TERMS);
}

static void plan() {
    Call c;
    c.bits[2] = 0, c.bits[3] = 13;   // the boolean's validity starts at bit 13
    uint8_t wide_valid[3] = {0, 0b01100000, 0};
    c.validity[1] = wide_valid;
    c.term_col[0] = 2, c.term_op[0] = OXH_FILTER_LT, c.lit_off[1] = c.lit_off[2] = 1;   // terms on c2, c1, c2: c0 is not named
    const filterrows::HostPlan p(c.a);
    EXPECT(p.idx_bytes == 16 && p.mask_bytes == 16);                    // 3 u32, one mask word; 16-B aligned each
    EXPECT(p.staged.size() == 2 && p.staged_of[0] == -1 && p.staged_of[2] == 0 && p.staged_of[1] == 1);
    EXPECT(p.staging.pieces.size() == 4);                               // offsets + span; bools + validity
    EXPECT(p.staging.pieces[0].at == 32);                               // behind idx and the mask
    const cols::Staged& text = p.staged[0];
    const cols::Staged& flag = p.staged[1];
    EXPECT(text.span_lo == 1 && p.staging.pieces[text.values].bytes == 5 && p.staging.pieces[text.offsets].bytes == 16);
    EXPECT(flag.nbit == 5 && p.staging.pieces[flag.validity].src == wide_valid + 1 && p.staging.pieces[flag.validity].bytes == 1);
    uint8_t* block = (uint8_t*)0x10000;
    EXPECT(p.staging.values_at(block, text) == block + p.staging.pieces[text.values].at - 1);
    EXPECT(p.staging.total % 16 == 0 && p.staging.total >= 32 + 4 * 16);
    for (const cols::Piece& piece : p.staging.pieces) EXPECT(piece.src != c.ints);
}

int main() {
    operators();
    kleene();
    bytes();
    fixed();
    arguments();
    lease();
    literals();
    plan();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
