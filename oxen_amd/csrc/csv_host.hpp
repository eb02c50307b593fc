// oxen_amd/csrc/csv_host.hpp -- the host-only pieces of oxh_csv_* (csv_read.hip): what the entries check before
// they need a device, in the header's order; the size of every working array; the class-bits-to-type rule of the
// inference; the header record's names; and the conversion of the float cells the device deferred. Plain C++ with
// no HIP in it, so that a stand-alone program can call it (tests/native/csv_host_test.cpp, which is also what a
// sanitizer build runs).
#pragma once

#include <locale.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <charconv>
#include <string>
#include <vector>

#include "../../include/oxen_hash.h"
#include "csv_number.hpp"

namespace oxh::csv {

constexpr uint64_t kMaxBytes = 1ull << 32;      // positions are u32: a buffer of 2^32 bytes and more is refused
constexpr uint32_t kTileBytes = 4096;           // one workgroup tile of the index kernels: 256 lanes x 16 bytes
constexpr uint32_t kLongCell = 512;             // a string cell of this many bytes and more is a whole wave's
constexpr uint32_t kDeferSlot = 48;             // bytes of a deferred cell's text that come down in its slot
constexpr uint64_t kBytes32Max = 0x7FFFFFFFull; // the most bytes of an OXH_CSV_STRING column (int32 offsets)
constexpr uint64_t kCtrlBytes = 256;

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
inline uint64_t blocks_of(uint64_t n) { return (n + 63) / 64; }          // 64-row blocks: one ballot word each
inline uint64_t scan_tiles_of(uint64_t n) { return (n + 2047) / 2048; }  // keyed_diff.hip's scan_tiles (checked where a lease is made)
// Tiles of the index kernels over `nbytes` at `misalign` = d_bytes & 15: they walk the 16-byte aligned space from
// d_bytes - misalign up to and including the position one past the last byte, where the last record may end.
inline uint64_t tiles_of(uint64_t misalign, uint64_t nbytes) { return (misalign + nbytes + 1 + kTileBytes - 1) / kTileBytes; }

inline bool known_type(uint32_t t) { return t >= OXH_CSV_INT64 && t <= OXH_CSV_STRING64; }
inline bool is_string(uint32_t t) { return t == OXH_CSV_STRING || t == OXH_CSV_STRING64; }
// bytes of the values buffer of a column of nrows rows that is not a string column
inline uint64_t fixed_value_bytes(uint32_t type, uint64_t nrows) { return type == OXH_CSV_BOOL ? (nrows + 7) / 8 : nrows * 8; }

// "" when oxh_csv_open_*'s arguments are well formed, else what is wrong with them, in the header's order.
inline std::string open_error(const uint8_t* bytes, uint64_t nbytes, uint32_t separator, uint32_t quote, uint32_t flags,
                              void* const* out, const uint64_t* stats8) {
    if (separator > 255) return "the separator is not one byte";
    if (quote > OXH_CSV_NO_QUOTE) return "the quote is neither one byte nor OXH_CSV_NO_QUOTE";
    if (separator == '\n' || separator == '\r') return "the separator is a line end";
    if (quote == '\n' || quote == '\r') return "the quote is a line end";
    if (quote == separator) return "the quote is the separator";
    if (flags & ~(uint32_t)OXH_CSV_HAS_HEADER) return "unknown flags";
    if (nbytes >= kMaxBytes) return "a buffer of 2^32 bytes and more (positions are u32)";
    if (nbytes && !bytes) return "bytes is NULL";
    if (!out) return "out is NULL";
    if (!stats8) return "stats8 is NULL";
    return "";
}

struct ColumnsArgs {
    uint64_t nrows, ncols;  // of the handle
    uint32_t nsel;
    const uint32_t* col_idx;
    const uint32_t* types;
    const uint64_t* value_capacity;
    void* const* values;
    void* const* offsets;
    uint8_t* const* validity;
    uint64_t* value_bytes;
    uint64_t* stats4;
};

// The same for oxh_csv_columns_* (after the handle itself was checked). All three output tables NULL: the call
// only measures.
inline std::string columns_error(const ColumnsArgs& a) {
    if (a.nsel && (!a.col_idx || !a.types)) return "col_idx or types is NULL";
    for (uint32_t k = 0; k < a.nsel; ++k)
        if (a.col_idx[k] >= a.ncols) return "selection " + std::to_string(k) + " names column " + std::to_string(a.col_idx[k]) + " of " + std::to_string(a.ncols);
    for (uint32_t k = 0; k < a.nsel; ++k)
        if (!known_type(a.types[k])) return "selection " + std::to_string(k) + " has unknown type " + std::to_string(a.types[k]);
    if (a.nsel && (!a.value_bytes || !a.stats4)) return "value_bytes or stats4 is NULL";
    const bool measure = !a.values && !a.offsets && !a.validity;
    if (measure || !a.nsel) return "";
    if (!a.values || !a.offsets || !a.validity) return "only some of values, offsets and validity are NULL";
    if (!a.value_capacity) return "value_capacity is NULL with outputs";
    if (!a.nrows) return "";
    for (uint32_t k = 0; k < a.nsel; ++k) {
        const std::string col = "selection " + std::to_string(k);
        if (!a.validity[k]) return col + " has no validity buffer";
        if (is_string(a.types[k])) {
            if (!a.offsets[k]) return col + " is a string column without offsets";
            if (!a.values[k] && a.value_capacity[k]) return col + " has a capacity but no values";
            if ((uintptr_t)a.offsets[k] & (a.types[k] == OXH_CSV_STRING64 ? 7 : 3)) return col + ": offsets is not aligned to its entries";
        } else {
            if (!a.values[k]) return col + " has no values buffer";
            if (a.value_capacity[k] < fixed_value_bytes(a.types[k], a.nrows))
                return col + ": value_capacity is below the " + std::to_string(fixed_value_bytes(a.types[k], a.nrows)) + " bytes of its values";
            if (a.types[k] != OXH_CSV_BOOL && ((uintptr_t)a.values[k] & 7)) return col + ": values is not 8-byte aligned";
        }
    }
    return "";
}

// What a string column's measured bytes allow ("" = fine): int32 offsets hold 2^31 - 1 at most, as in the take,
// and the caller's buffer holds value_capacity.
inline std::string string_bytes_error(uint32_t type, uint64_t bytes, bool write, uint64_t capacity) {
    if (type == OXH_CSV_STRING && bytes > kBytes32Max)
        return std::to_string(bytes) + " bytes in an OXH_CSV_STRING column (int32 offsets hold 2^31 - 1): ask for OXH_CSV_STRING64";
    if (write && bytes > capacity) return std::to_string(bytes) + " bytes of strings, value_capacity " + std::to_string(capacity);
    return "";
}

// The inference's rule over the AND of a column's class bits. A column whose cells are all empty has every bit
// and is a string column (`all_empty`).
inline uint32_t type_of_bits(uint32_t bits, bool all_empty) {
    if (all_empty) return OXH_CSV_STRING;
    if (bits & csvnum::kIntOk) return OXH_CSV_INT64;
    if (bits & csvnum::kFloatOk) return OXH_CSV_FLOAT64;
    if (bits & csvnum::kBoolOk) return OXH_CSV_BOOL;
    return OXH_CSV_STRING;
}

// ---------------------------------------------------------------- working memory (offsets into a lease)
struct Carver {
    uint64_t at = 0;
    uint64_t operator()(uint64_t bytes) {
        const uint64_t here = at;
        at += align256(bytes);
        return here;
    }
};

// open, first lease: per tile the quote count and its scan, the delimiter and record-end counts and their scans
// -- 36 B per 4 KiB tile -- and the three scans' tile sums.
struct IndexLease {
    uint64_t ctrl, quotes, quote_scan, delims, delim_scan, recs, rec_scan, quote_sums, delim_sums, rec_sums, total;
    explicit IndexLease(uint64_t tiles) {
        Carver carve;
        ctrl = carve(kCtrlBytes);
        quotes = carve(tiles * 4), quote_scan = carve(tiles * 8);
        delims = carve(tiles * 4), delim_scan = carve(tiles * 8);
        recs = carve(tiles * 4), rec_scan = carve(tiles * 8);
        const uint64_t sums = (scan_tiles_of(tiles) + 1) * 8;  // a scan's tile sums; the last word is its total
        quote_sums = carve(sums), delim_sums = carve(sums), rec_sums = carve(sums);
        total = carve.at;
    }
};

// open, second lease: per 64 records the kept records' mask word, their count and its scan (20 B per 64 records).
struct RowMapLease {
    uint64_t ctrl, mask, counts, bases, sums, total;
    explicit RowMapLease(uint64_t nrec) {
        const uint64_t blocks = blocks_of(nrec);
        Carver carve;
        ctrl = carve(kCtrlBytes);
        mask = carve(blocks * 8), counts = carve(blocks * 4), bases = carve(blocks * 8);
        sums = carve((scan_tiles_of(blocks) + 1) * 8);
        total = carve.at;
    }
};

// columns: 8 control words per selected column; one string column at a time: a length per row and its scan
// (12 B per row); per FLOAT64 column the deferred cells' mask word and count per 64 rows, and once their scan.
struct ColumnsLease {
    uint64_t ctrl, lens, len_scan, sums, defer_bases, total;
    std::vector<uint64_t> defer_mask, defer_counts;  // per selected column (0 where it is no FLOAT64 column)
    ColumnsLease(uint64_t nrows, uint32_t nsel, const uint32_t* types, bool write) : defer_mask(nsel, 0), defer_counts(nsel, 0) {
        bool strings = false, floats = false;
        for (uint32_t k = 0; k < nsel; ++k) strings |= is_string(types[k]), floats |= types[k] == OXH_CSV_FLOAT64;
        const uint64_t blocks = blocks_of(nrows);
        Carver carve;
        ctrl = carve((uint64_t)nsel * 64 + kCtrlBytes);
        lens = carve(strings && write ? nrows * 4 : 0), len_scan = carve(strings && write ? nrows * 8 : 0);
        sums = carve((scan_tiles_of(std::max(nrows, blocks)) + 1) * 8);
        defer_bases = carve(floats && write ? blocks * 8 : 0);
        for (uint32_t k = 0; k < nsel; ++k)
            if (types[k] == OXH_CSV_FLOAT64 && write) defer_mask[k] = carve(blocks * 8), defer_counts[k] = carve(blocks * 4);
        total = carve.at;
    }
};

// ---------------------------------------------------------------- field values on the host
// The value of a field whose bytes are [p, p + n): without its quotes when both ends are the quote, every doubled
// quote inside as one (left to right: of a run of k quotes, k / 2 are dropped).
inline std::string field_value(const uint8_t* p, uint32_t n, uint32_t quote) {
    if (!csvnum::strip_quotes(p, n, quote)) return std::string((const char*)p, n);
    std::string out;
    for (uint32_t i = 0; i < n; ++i) {
        out.push_back((char)p[i]);
        if (p[i] == quote && i + 1 < n && p[i + 1] == quote) ++i;
    }
    return out;
}

// The names of the header record. rec: its bytes, from `start` of the buffer; ends: the position of the end of
// each of its ncols fields (the last may have a '\r' before it, which is no part of the name).
inline void header_names(const uint8_t* rec, uint32_t start, const uint32_t* ends, uint32_t ncols, uint32_t quote,
                         std::vector<uint8_t>& names, std::vector<uint64_t>& offsets) {
    names.clear(), offsets.assign(1, 0);
    uint32_t from = start;
    for (uint32_t c = 0; c < ncols; ++c) {
        uint32_t to = ends[c];
        if (c + 1 == ncols && to > from && rec[to - 1 - start] == '\r') --to;
        const std::string v = field_value(rec + (from - start), to - from, quote);
        names.insert(names.end(), v.begin(), v.end());
        offsets.push_back(names.size());
        from = ends[c] + 1;
    }
}

// ---------------------------------------------------------------- deferred floats
// The double nearest to the text of a cell that matched the FLOAT64 grammar: std::from_chars (locale-free,
// correctly rounded); a value outside the doubles (from_chars leaves it unset) through strtod in the "C" locale,
// which gives the signed infinity or zero (or the subnormal) that rounding gives.
inline double convert_deferred(const char* p, size_t n) {
    bool neg = false;
    if (n && (*p == '+' || *p == '-')) neg = *p == '-', ++p, --n;
    double v = 0.0;
    const std::from_chars_result r = std::from_chars(p, p + n, v, std::chars_format::general);
    if (r.ec != std::errc() || r.ptr != p + n) {
        static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
        const std::string text(p, n);
        v = c_locale ? strtod_l(text.c_str(), nullptr, c_locale) : strtod(text.c_str(), nullptr);
    }
    return neg ? -v : v;
}

}  // namespace oxh::csv
