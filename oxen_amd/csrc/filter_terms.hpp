// oxen_amd/csrc/filter_terms.hpp -- the terms of a row filter (filter_rows.hip: oxh_filter_rows_*; the
// semantics are stated in include/oxen_hash.h). Callable on the host and on the device, so that the
// stand-alone program tests/native/filter_rows_host_test.cpp checks the very code the kernel runs.
//
// A filter is terms `column OP literal` joined by && / ||, folded left to right with no precedence. One term
// on one row is three-valued:
//   null    the cell is null -- for every operator, != included;
//   else    holds(op, cmp) with cmp = -1 / 0 / 1 for cell < / == / > literal:
//           fixed-width cells by sort_keys.hpp's fixed_word of the cell against the same word of the literal
//           (signed / unsigned by the order class; floats numeric, -0.0 == +0.0, every NaN equal to every
//           NaN and above +inf), booleans false < true, byte cells unsigned byte-wise lexicographic with a
//           proper prefix first ("" is a value).
// && and || are Kleene's: null && false = false, null || true = true, else a null is contagious. A row is
// selected exactly when the folded result is true.
#pragma once

#include <stdint.h>
#include <string.h>

#include "sort_keys.hpp"

namespace oxh::filterterms {

// OXH_FILTER_EQ .. OXH_FILTER_GE are 0 .. 5 in this order; OXH_FILTER_AND 0, OXH_FILTER_OR 1
constexpr uint32_t kOps = 6;
constexpr uint32_t kFalse = 0, kTrue = 1, kNull = 2;  // a term's, and the fold's, result

OXH_SORT_HD bool known_op(uint32_t op) { return op < kOps; }
OXH_SORT_HD bool known_logical(uint32_t op) { return op == OXH_FILTER_AND || op == OXH_FILTER_OR; }

// the low `width` bytes of a literal's word (width 1, 4 or 8)
OXH_SORT_HD uint64_t low_bytes(uint64_t word, uint32_t width) { return width >= 8 ? word : word & ((1ull << (8 * width)) - 1); }

OXH_SORT_HD int compare_words(uint64_t a, uint64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

// raw cell against raw literal (little-endian bytes, zero-extended) of a fixed-width column
OXH_SORT_HD int compare_fixed(uint32_t order, uint32_t width, uint64_t cell, uint64_t lit) {
    return compare_words(sortkeys::fixed_word(order, width, cell), sortkeys::fixed_word(order, width, low_bytes(lit, width)));
}

OXH_SORT_HD uint64_t load8(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// -1 / 0 / 1: the byte cell against the literal, unsigned byte-wise, a proper prefix first. Reads only
// cell[0 .. min(len, litlen)) and lit[0 .. min(len, litlen)), eight bytes at a time where that span allows.
OXH_SORT_HD int compare_bytes(const uint8_t* cell, uint64_t len, const uint8_t* lit, uint64_t litlen) {
    const uint64_t common = len < litlen ? len : litlen;
    uint64_t b = 0;
    for (; b + 8 <= common; b += 8) {
        const uint64_t x = load8(cell + b), y = load8(lit + b);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;  // the first byte that differs decides
    }
    for (; b < common; ++b)
        if (cell[b] != lit[b]) return cell[b] < lit[b] ? -1 : 1;
    return compare_words(len, litlen);
}

// The same for a term with operator `op`: == and != on cells of another length are decided without a byte read.
OXH_SORT_HD int compare_bytes_for(uint32_t op, const uint8_t* cell, uint64_t len, const uint8_t* lit, uint64_t litlen) {
    if ((op == OXH_FILTER_EQ || op == OXH_FILTER_NE) && len != litlen) return 1;  // "not equal" is all they ask
    return compare_bytes(cell, len, lit, litlen);
}

// Does `cell OP literal` hold, given cmp = -1 / 0 / 1?
OXH_SORT_HD bool holds(uint32_t op, int cmp) {
    switch (op) {
        case OXH_FILTER_EQ: return cmp == 0;
        case OXH_FILTER_NE: return cmp != 0;
        case OXH_FILTER_LT: return cmp < 0;
        case OXH_FILTER_LE: return cmp <= 0;
        case OXH_FILTER_GT: return cmp > 0;
        default: return cmp >= 0;  // OXH_FILTER_GE
    }
}

// a present cell's term
OXH_SORT_HD uint32_t term_result(uint32_t op, int cmp) { return holds(op, cmp) ? kTrue : kFalse; }

OXH_SORT_HD uint32_t and3(uint32_t a, uint32_t b) {
    if (a == kFalse || b == kFalse) return kFalse;
    return a == kNull || b == kNull ? kNull : kTrue;
}
OXH_SORT_HD uint32_t or3(uint32_t a, uint32_t b) {
    if (a == kTrue || b == kTrue) return kTrue;
    return a == kNull || b == kNull ? kNull : kFalse;
}

// One step of the fold: `sofar` joined with term t's result (t >= 1) by logical operator t - 1, which is bit
// t - 1 of `or_bits` (set: ||).
OXH_SORT_HD uint32_t fold_step(uint32_t sofar, uint32_t result, uint32_t t, uint32_t or_bits) {
    return (or_bits >> (t - 1)) & 1 ? or3(sofar, result) : and3(sofar, result);
}

// The fold over a row's term results, left to right with no precedence: a || b && c is (a || b) && c.
OXH_SORT_HD uint32_t fold(const uint32_t* results, uint32_t nterms, uint32_t or_bits) {
    uint32_t sofar = results[0];
    for (uint32_t t = 1; t < nterms; ++t) sofar = fold_step(sofar, results[t], t, or_bits);
    return sofar;
}

}  // namespace oxh::filterterms
