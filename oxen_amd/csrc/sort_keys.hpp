// oxen_amd/csrc/sort_keys.hpp -- the order-preserving key words of the row sort (sort_rows.hip:
// oxh_sort_rows_*; the order itself is stated in include/oxen_hash.h). Callable on the host and on the
// device, so that the stand-alone program tests/native/sort_rows_host_test.cpp checks the very code the
// kernels run: for two cells a, b of one column, a sorts before b exactly when triple(a) < triple(b).
//
// One refinement round looks at one piece of a row's key: the cell of the key column under the row's
// cursor, or -- for a byte column -- one 8-byte chunk of it. That piece is the triple (class, word, tail):
//   class   null < exhausted < present. "Exhausted": a byte cell with no byte left at this chunk ("" at
//           chunk 0, "abcdefgh" at chunk 1), so a proper prefix comes first and a null before "".
//   word    fixed-width: the value's bits made unsigned-comparable (sign bit flipped for a signed value;
//           the usual total-order transform of a float after -0.0 became +0.0 and every NaN one NaN above
//           +inf; a boolean's 0 / 1). Byte cells: the chunk's bytes big-endian, zero-padded to 8.
//   tail    the real bytes in a byte cell's chunk, 1..8 (0 for everything else): what orders "a" before
//           "a\0", whose words are equal.
// A chunk with tail 8 is followed by the next chunk of the same cell; every other triple ends its column.
#pragma once

#include <stdint.h>

#include "../../include/oxen_hash.h"

#if defined(__HIPCC__)
#define OXH_SORT_HD __host__ __device__ __forceinline__
#else
#define OXH_SORT_HD inline
#endif

namespace oxh::sortkeys {

constexpr uint32_t kClassNull = 0, kClassExhausted = 1, kClassPresent = 2;
constexpr uint32_t kChunk = 8;  // bytes of a byte cell one round looks at

struct Triple {
    uint32_t cls;
    uint32_t tail;
    uint64_t word;
};

OXH_SORT_HD bool less(const Triple& a, const Triple& b) {
    if (a.cls != b.cls) return a.cls < b.cls;
    if (a.word != b.word) return a.word < b.word;
    return a.tail < b.tail;
}
OXH_SORT_HD bool same(const Triple& a, const Triple& b) { return a.cls == b.cls && a.word == b.word && a.tail == b.tail; }

// raw: the cell's little-endian bytes, zero-extended; width 1, 4 or 8
OXH_SORT_HD uint64_t encode_signed(uint64_t raw, uint32_t width) { return raw ^ (1ull << (8 * width - 1)); }
OXH_SORT_HD uint64_t encode_unsigned(uint64_t raw) { return raw; }
OXH_SORT_HD uint64_t encode_float32(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = 0x7FC00000u;  // every NaN: one NaN, above +inf
    if (bits == 0x80000000u) bits = 0;                          // -0.0 equals +0.0
    return (bits & 0x80000000u) ? (uint32_t)~bits : (bits | 0x80000000u);
}
OXH_SORT_HD uint64_t encode_float64(uint64_t bits) {
    if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) bits = 0x7FF8000000000000ull;
    if (bits == 0x8000000000000000ull) bits = 0;
    return (bits & 0x8000000000000000ull) ? ~bits : (bits | 0x8000000000000000ull);
}

// The word of a present fixed-width cell. order: OXH_SORT_*; OXH_SORT_FLOAT needs width 4 or 8.
OXH_SORT_HD uint64_t fixed_word(uint32_t order, uint32_t width, uint64_t raw) {
    if (order == OXH_SORT_SIGNED) return encode_signed(raw, width);
    if (order == OXH_SORT_FLOAT) return width == 4 ? encode_float32((uint32_t)raw) : encode_float64(raw);
    return encode_unsigned(raw);
}

OXH_SORT_HD Triple null_triple() { return Triple{kClassNull, 0, 0}; }
OXH_SORT_HD Triple fixed_triple(uint32_t order, uint32_t width, uint64_t raw) {
    return Triple{kClassPresent, 0, fixed_word(order, width, raw)};
}
OXH_SORT_HD Triple bool_triple(bool v) { return Triple{kClassPresent, 0, v ? 1ull : 0ull}; }

// Chunk `chunk` of a present byte cell of `len` bytes at `cell`. Reads only cell[8 * chunk .. min(len, 8 * chunk + 8)).
OXH_SORT_HD Triple bytes_triple(const uint8_t* cell, uint64_t len, uint64_t chunk) {
    if (chunk > len / kChunk || chunk * kChunk >= len) return Triple{kClassExhausted, 0, 0};
    const uint64_t at = chunk * kChunk, left = len - at;
    const uint32_t take = left < kChunk ? (uint32_t)left : kChunk;
    uint64_t word = 0;
    for (uint32_t b = 0; b < take; ++b) word |= (uint64_t)cell[at + b] << (56 - 8 * b);
    return Triple{kClassPresent, take, word};
}

// Does the row stay in this column (the next chunk of the same cell) after a round that saw `t`?
OXH_SORT_HD bool next_chunk(const Triple& t) { return t.cls == kClassPresent && t.tail == kChunk; }

// The second key word of a round: tail in byte 0, class in byte 1, the tie-group id from byte 2 up. A stable
// sort by byte 0, then by the word's eight bytes, then by bytes 1.. of this one orders by (group, class, word, tail).
OXH_SORT_HD uint64_t pack_meta(uint32_t group, const Triple& t) { return (uint64_t)group << 16 | (uint64_t)t.cls << 8 | t.tail; }
OXH_SORT_HD uint32_t meta_tail(uint64_t meta) { return (uint32_t)(meta & 0xFF); }
OXH_SORT_HD uint32_t meta_class(uint64_t meta) { return (uint32_t)(meta >> 8 & 0xFF); }

}  // namespace oxh::sortkeys
