// oxen_amd/csrc/concat_columns_host.hpp -- the host-only pieces of oxh_concat_columns_* (concat_columns.hip):
// what both forms check before they need a device, the prefix table of rows, the descriptors and the item
// lists the kernels walk, the sizes the host form knows from its own offsets and its staging plan. Plain C++
// with no HIP in it, so that a stand-alone program can call it (tests/native/concat_columns_host_test.cpp,
// which is also what a sanitizer build runs). The staging of a column is columns.hpp's.
#pragma once

#include "columns.hpp"

namespace oxh::concat {

constexpr uint64_t kMaxRows = 0xFFFFFFFEull;     // as the take: the output is a frame the take can index
constexpr uint64_t kMaxBytes32 = 0x7FFFFFFFull;  // what an int32 offset can say
// One copy item: the 16-byte blocks of the destination that one aligned window of this many bytes holds (a
// workgroup stores 4 KiB per step). One rebase item: this many offsets.
constexpr uint32_t kConcatPiece = 16384;
constexpr uint32_t kConcatOffsetPiece = 4096;

struct Args {
    uint32_t nparts, ncols;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint64_t* part_rows;
    const uint64_t* first;
    const uint64_t* count;
    const uint64_t* value_capacity;
    void* const* out_values;
    void* const* out_offsets;
    uint8_t* const* out_validity;
    uint64_t* value_bytes;
    uint32_t* written;
};

inline uint64_t first_of(const Args& a, uint32_t p) { return a.count ? a.first[p] : 0; }
inline uint64_t count_of(const Args& a, uint32_t p) { return a.count ? a.count[p] : a.part_rows[p]; }
inline bool sizes_only(const Args& a) { return !a.out_values && !a.out_offsets && !a.out_validity; }
inline uint64_t bitmap_bytes(uint64_t rows) { return (rows + 7) >> 3; }
inline uint64_t plain_value_bytes(uint32_t kind, uint64_t rows) {
    return kind == OXH_COL_BOOL ? bitmap_bytes(rows) : rows * cols::width_of(kind);
}

// row_base[p] = the output row of part p's first taken row; row_base[nparts] = N. (After argument_error.)
inline std::vector<uint64_t> row_table(const Args& a) {
    std::vector<uint64_t> base((size_t)a.nparts + 1, 0);
    for (uint32_t p = 0; p < a.nparts; ++p) base[p + 1] = base[p] + count_of(a, p);
    return base;
}

// "" when the arguments are well formed, else what is wrong with them (the order is the header's).
// host: the offsets can be read and are checked; else the outputs are device memory and the bit-packed ones
// must be 8-byte aligned.
inline std::string argument_error(const Args& a, bool host) {
    if (!a.kinds || !a.values || !a.offsets || !a.validity || !a.bit_offsets || !a.part_rows || (a.count && !a.first))
        return "kinds, values, offsets, validity, bit_offsets, part_rows or (with count) first is NULL";
    if (a.nparts == 0 || a.ncols == 0) return "nparts or ncols is 0";
    if (a.nparts > OXH_CONCAT_MAX_PARTS) return "more than OXH_CONCAT_MAX_PARTS parts";
    for (uint32_t c = 0; c < a.ncols; ++c)
        if (!cols::known_kind(a.kinds[c])) return "column " + std::to_string(c) + " has unknown kind " + std::to_string(a.kinds[c]);
    for (uint32_t p = 0; p < a.nparts; ++p)
        if (first_of(a, p) > a.part_rows[p] || count_of(a, p) > a.part_rows[p] - first_of(a, p))
            return "part " + std::to_string(p) + ": first + count is above its rows";
    uint64_t n = 0;
    for (uint32_t p = 0; p < a.nparts; ++p) {
        if (a.part_rows[p] > kMaxRows) return "part " + std::to_string(p) + " has more than 2^32 - 2 rows";
        n += count_of(a, p);  // each at most 2^32 - 2, at most 65 536 of them
        if (n > kMaxRows) return "more than 2^32 - 2 output rows";
    }
    if (!a.value_bytes || !a.written) return "value_bytes or written is NULL";
    auto at = [&](uint32_t p, uint32_t c) { return (size_t)p * a.ncols + c; };
    for (uint32_t p = 0; p < a.nparts; ++p)
        for (uint32_t c = 0; c < a.ncols && count_of(a, p); ++c)
            if (cols::is_bytes(a.kinds[c]) && !a.offsets[at(p, c)])
                return "part " + std::to_string(p) + " column " + std::to_string(c) + " is a byte column without offsets";
    for (uint32_t p = 0; p < a.nparts; ++p)
        for (uint32_t c = 0; c < a.ncols && count_of(a, p); ++c)
            if (!cols::is_bytes(a.kinds[c]) && !a.values[at(p, c)])
                return "part " + std::to_string(p) + " column " + std::to_string(c) + " has no values";
    if (!sizes_only(a)) {
        if (!a.out_values || !a.out_offsets || !a.out_validity) return "some of out_values, out_offsets, out_validity are NULL and some are not";
        if (!a.value_capacity) return "outputs without value_capacity";
        for (uint32_t c = 0; c < a.ncols; ++c) {
            const uint32_t kind = a.kinds[c];
            const std::string out = "output column " + std::to_string(c);
            if (cols::is_bytes(kind) && !a.out_offsets[c]) return out + " is a byte column without out_offsets";
            if (!n) continue;
            if (!a.out_validity[c]) return out + " has no out_validity";
            if (!cols::is_bytes(kind) && !a.out_values[c]) return out + " has no out_values";
            if (cols::is_bytes(kind) && a.value_capacity[c] && !a.out_values[c]) return out + " has value_capacity but no out_values";
            if (!host && (((uintptr_t)a.out_validity[c] & 7) || (kind == OXH_COL_BOOL && ((uintptr_t)a.out_values[c] & 7))))
                return out + ": a bit-packed output is not 8-byte aligned";
        }
    }
    if (!host) return "";  // the spans are on the device: the kernels check them
    for (uint32_t p = 0; p < a.nparts; ++p)
        for (uint32_t c = 0; c < a.ncols && count_of(a, p); ++c) {
            const uint32_t kind = a.kinds[c];
            if (!cols::is_bytes(kind)) continue;
            const void* off = (const uint8_t*)a.offsets[at(p, c)] + first_of(a, p) * cols::offset_width(kind);
            const std::string what =
                cols::column_error("part " + std::to_string(p) + " column " + std::to_string(c), kind, a.values[at(p, c)], off, count_of(a, p), true);
            if (!what.empty()) return what;
        }
    return "";
}

// ---------------------------------------------------------------- what the kernels walk
// One part's source of a bit-packed output (a validity bitmap, a boolean's values): `bit` is the bit of the
// part's first taken row; p NULL = all ones (a part without validity). Stream s of the call (s < ncols: the
// validity of column s; then the values of the boolean columns in column order) has its parts at
// table[s * nparts + p].
struct BitSrc {
    const uint8_t* p;
    uint64_t bit;
};

// A range of one output buffer that comes from one part.
//   mode 0      copy: dst[0, n) = src[0, n) bytes (fixed-width values, a byte column's span);
//   mode 4 / 8  rebase: n offsets of that width, element j of dst = base + clamp(v_j, lo, hi) - lo, where
//               v_0 = src[0] and v_j = src[j] but src[j - 1] when the pair (src[j - 1], src[j]) is negative or
//               decreases (that cell then has length 0). src is the part's offsets at its first taken row.
struct Span {
    const uint8_t* src;
    uint8_t* dst;
    uint64_t n;
    int64_t lo, hi;
    uint64_t base;
    uint32_t mode, pad;
};

struct Item {
    uint64_t span;   // which Span
    uint32_t piece;  // which piece of it
    uint32_t pad;
};

// Copy pieces are windows of kConcatPiece bytes aligned ON THE DESTINATION's 16-byte grid: piece k holds
// the blocks [A + k * kConcatPiece, A + (k + 1) * kConcatPiece) with A = dst rounded down to 16.
inline uint64_t span_pieces(const Span& s) {
    if (!s.n) return 0;
    if (s.mode) return (s.n + kConcatOffsetPiece - 1) / kConcatOffsetPiece;
    return (((uintptr_t)s.dst & 15) + s.n + kConcatPiece - 1) / kConcatPiece;
}

inline void add_items(std::vector<Item>& items, const std::vector<Span>& spans, size_t from) {
    for (size_t s = from; s < spans.size(); ++s)
        for (uint64_t k = 0, n = span_pieces(spans[s]); k < n; ++k) items.push_back({(uint64_t)s, (uint32_t)k, 0});
}

// A byte column's part: [lo, hi) = (offsets[first], offsets[first + count]) as read; a span that is negative
// or decreases is bad and holds no bytes.
struct ByteSpan {
    int64_t lo = 0, hi = 0;
    bool bad() const { return lo < 0 || hi < lo; }
    uint64_t bytes() const { return bad() ? 0 : (uint64_t)(hi - lo); }
};

// The plan of one call over sources at `values` / `offsets` / `validity` (the ABI's tables; device addresses
// in the device path): row_base, the bit streams, and -- once the byte spans are known -- the sizes, then,
// given the outputs, the spans and the two item lists.
struct Plan {
    std::vector<uint64_t> row_base;
    uint64_t n = 0;
    std::vector<uint32_t> byte_cols, bool_cols;
    std::vector<BitSrc> bits;         // (ncols + bool_cols.size()) * nparts
    std::vector<ByteSpan> byte_span;  // byte_cols.size() * nparts: [j * nparts + p]
    std::vector<uint64_t> need;       // value bytes of every column
    std::vector<Span> spans;
    std::vector<Item> fixed_items, byte_items;  // the fixed-width copies and the rebases; the byte columns' copies
    bool bad_span = false;

    explicit Plan(const Args& a) : row_base(row_table(a)), n(row_base.back()), need(a.ncols, 0) {
        for (uint32_t c = 0; c < a.ncols; ++c) {
            if (cols::is_bytes(a.kinds[c])) byte_cols.push_back(c);
            else need[c] = plain_value_bytes(a.kinds[c], n);
            if (a.kinds[c] == OXH_COL_BOOL) bool_cols.push_back(c);
        }
        byte_span.resize(byte_cols.size() * (size_t)a.nparts);
    }
    uint32_t nstreams(const Args& a) const { return a.ncols + (uint32_t)bool_cols.size(); }

    void make_bits(const Args& a) {
        bits.assign((size_t)nstreams(a) * a.nparts, BitSrc{nullptr, 0});
        for (uint32_t p = 0; p < a.nparts; ++p) {
            if (!count_of(a, p)) continue;
            for (uint32_t c = 0; c < a.ncols; ++c) {
                const size_t at = (size_t)p * a.ncols + c;
                bits[(size_t)c * a.nparts + p] = {a.validity[at], a.bit_offsets[2 * at + 1] + first_of(a, p)};
            }
            for (size_t j = 0; j < bool_cols.size(); ++j) {
                const size_t at = (size_t)p * a.ncols + bool_cols[j];
                bits[(a.ncols + j) * a.nparts + p] = {(const uint8_t*)a.values[at], a.bit_offsets[2 * at] + first_of(a, p)};
            }
        }
    }

    // need[] of the byte columns from byte_span; "" or why the call stops here.
    std::string make_sizes(const Args& a) {
        bad_span = false;
        for (size_t j = 0; j < byte_cols.size(); ++j) {
            uint64_t total = 0;
            for (uint32_t p = 0; p < a.nparts; ++p) {
                const ByteSpan& s = byte_span[j * a.nparts + p];
                if (!count_of(a, p)) continue;
                bad_span |= s.bad();
                if (s.bytes() && !a.values[(size_t)p * a.ncols + byte_cols[j]])
                    return "part " + std::to_string(p) + " column " + std::to_string(byte_cols[j]) + " has bytes but no values";
                total += s.bytes();
            }
            need[byte_cols[j]] = total;
            if (a.kinds[byte_cols[j]] == OXH_COL_BYTES32 && total > kMaxBytes32)
                return "output column " + std::to_string(byte_cols[j]) + " holds " + std::to_string(total) +
                       " B, more than int32 offsets can say: pass the column as OXH_COL_BYTES64";
        }
        return "";
    }

    bool fits(const Args& a) const {
        for (uint32_t c : byte_cols)
            if (need[c] > a.value_capacity[c]) return false;
        return true;
    }

    // The spans and item lists of the write into out_values / out_offsets (n > 0).
    void make_items(const Args& a, void* const* out_values, void* const* out_offsets) {
        spans.clear(), fixed_items.clear(), byte_items.clear();
        uint32_t last = 0;  // the last part with rows writes off[N] too
        for (uint32_t p = 0; p < a.nparts; ++p)
            if (count_of(a, p)) last = p;
        for (uint32_t c = 0; c < a.ncols; ++c) {
            const uint32_t w = cols::width_of(a.kinds[c]);
            if (!w) continue;
            for (uint32_t p = 0; p < a.nparts; ++p)
                if (const uint64_t cnt = count_of(a, p))
                    spans.push_back({(const uint8_t*)a.values[(size_t)p * a.ncols + c] + first_of(a, p) * w,
                                     (uint8_t*)out_values[c] + row_base[p] * w, cnt * w, 0, 0, 0, 0, 0});
        }
        std::vector<Span> copies;
        for (size_t j = 0; j < byte_cols.size(); ++j) {
            const uint32_t c = byte_cols[j], ow = cols::offset_width(a.kinds[c]);
            uint64_t base = 0;
            for (uint32_t p = 0; p < a.nparts; ++p) {
                const uint64_t cnt = count_of(a, p);
                if (!cnt) continue;
                const ByteSpan& s = byte_span[j * a.nparts + p];
                const int64_t lo = s.bad() ? 0 : s.lo, hi = s.bad() ? 0 : s.hi;
                const size_t at = (size_t)p * a.ncols + c;
                spans.push_back({(const uint8_t*)a.offsets[at] + first_of(a, p) * ow, (uint8_t*)out_offsets[c] + row_base[p] * ow,
                                 cnt + (p == last ? 1 : 0), lo, hi, base, ow, 0});
                if (s.bytes()) copies.push_back({(const uint8_t*)a.values[at] + lo, (uint8_t*)out_values[c] + base, s.bytes(), 0, 0, 0, 0, 0});
                base += s.bytes();
            }
        }
        add_items(fixed_items, spans, 0);
        const size_t from = spans.size();
        spans.insert(spans.end(), copies.begin(), copies.end());
        add_items(byte_items, spans, from);
    }
};

// ---------------------------------------------------------------- the host form
// The byte spans from the caller's own offsets (argument_error(host = true) passed: none is bad).
inline void host_spans(const Args& a, Plan& plan) {
    for (size_t j = 0; j < plan.byte_cols.size(); ++j)
        for (uint32_t p = 0; p < a.nparts; ++p) {
            if (!count_of(a, p)) continue;
            const uint32_t kind = a.kinds[plan.byte_cols[j]];
            const void* off = a.offsets[(size_t)p * a.ncols + plan.byte_cols[j]];
            plan.byte_span[j * a.nparts + p] = {cols::offset_at(off, kind, first_of(a, p)), cols::offset_at(off, kind, first_of(a, p) + count_of(a, p))};
        }
}

// The host form's input block: for every part and column only the taken range (columns.hpp's staging of a
// column of count rows that starts at the part's first taken row). staged[p * ncols + c].
struct HostStaging {
    cols::Staging block;
    std::vector<cols::Staged> staged;
    explicit HostStaging(const Args& a) : staged((size_t)a.nparts * a.ncols) {
        for (uint32_t p = 0; p < a.nparts; ++p) {
            const uint64_t first = first_of(a, p), cnt = count_of(a, p);
            for (uint32_t c = 0; c < a.ncols && cnt; ++c) {
                const size_t at = (size_t)p * a.ncols + c;
                const uint32_t kind = a.kinds[c];
                const uint8_t* values = (const uint8_t*)a.values[at];
                if (cols::width_of(kind)) values += first * cols::width_of(kind);
                const uint8_t* offsets = cols::is_bytes(kind) ? (const uint8_t*)a.offsets[at] + first * cols::offset_width(kind) : nullptr;
                staged[at] = block.add_column(kind, values, offsets, a.validity[at], a.bit_offsets[2 * at] + first,
                                              a.bit_offsets[2 * at + 1] + first, cnt);
            }
        }
    }
};

// The host form's output block, as the take lays it out: at[3 * c + {0, 1, 2}] = validity, values, offsets.
struct OutBlock {
    std::vector<uint64_t> at;
    uint64_t total = 0;
    OutBlock(const Args& a, uint64_t n, const uint64_t* value_bytes) : at(3 * (size_t)a.ncols, 0) {
        auto add = [&](uint64_t bytes) {
            const uint64_t here = total;
            total += (bytes + 15) & ~15ull;
            return here;
        };
        for (uint32_t c = 0; c < a.ncols; ++c) {
            at[3 * c] = add(bitmap_bytes(n));
            at[3 * c + 1] = add(value_bytes[c]);
            at[3 * c + 2] = add(cols::is_bytes(a.kinds[c]) ? (n + 1) * cols::offset_width(a.kinds[c]) : 0);
        }
    }
};

}  // namespace oxh::concat
