// oxen_amd/csrc/parquet_host.hpp -- the host-only pieces of oxh_write_parquet_* (parquet_write.hip): the argument
// checks that need no device, in the header's order; the Thrift compact encoder; the planner that turns the measure
// kernel's tile table into pages, row groups, every PageHeader's bytes, every page's place in the file and the
// footer; the folding of the tiles' min / max partials into a column chunk's statistics; and for OXH_PARQUET_DICTIONARY
// the limits, the fallback decision, the index width and the index stream's bytes; and for the list columns of
// oxh_write_parquet_lists_* (parquet_write_lists.hip) their argument checks, the level streams' heads, their pages cut
// by level entries and their three schema elements. The format is stated in
// include/oxen_hash.h "Parquet". Plain C++ with no HIP in it, so that a stand-alone program can call it
// (tests/native/parquet_host_test.cpp, which is also what a sanitizer build runs).
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "columns.hpp"

namespace oxh::parquet {

constexpr uint64_t kTileRows = 1024;                 // rows are cut at its multiples
constexpr uint64_t kDefaultGroupRows = 1048576;
constexpr uint64_t kDefaultPageBytes = 1048576;
constexpr uint64_t kMaxRows = 1ull << 40;
constexpr uint64_t kMaxCell = 1ull << 32;            // a BYTE_ARRAY's length is a u32
constexpr uint64_t kMaxPage = 0x7FFFFFFFull;         // PageHeader's sizes are i32
constexpr uint32_t kFlagSnappy = 2;                  // OXH_PARQUET_SNAPPY: every page body is one raw Snappy block
constexpr uint32_t kFlagDictionary = 4;              // OXH_PARQUET_DICTIONARY: RLE_DICTIONARY chunks where the data allow
constexpr uint64_t kDictMaxEntries = 65536;          // a chunk of more distinct values stays PLAIN
constexpr uint64_t kDictMaxCell = 256;               // so does a chunk with a longer string cell
constexpr uint64_t kDictMaxPage = 1048576;           // and one whose dictionary page body is larger
constexpr const char* kCreatedBy = "oxen_amd parquet writer (gfx950)";

// What the measure kernel leaves per (tile, column), entry tile * ncols + column.
struct Tile {
    uint64_t value_bytes;  // 8 * valid; strings: the sum of 4 + length over the valid rows; booleans: valid
    uint64_t min, max;     // INT64: signed; DOUBLE: the bits, over the cells that are not NaN; BOOLEAN: min = bool_tail
                           // of the tile, the values of its last 7 valid rows
    uint32_t valid;        // the rows that are not null
    uint32_t has_minmax;   // min and max hold a value
};

// What the emit kernel reads per page and per (tile, column).
struct Page {
    uint64_t file_at;       // where the page's header starts in the file
    uint64_t head_src;      // its head in the plan's byte blob: PageHeader, the levels' length and run header
    uint64_t values_bytes;
    uint64_t row0;          // the page's first row
    uint32_t rows, nvalid;
    uint32_t head_len;
    uint32_t level_bytes;   // the bit-packed validity behind the head; 0 for a page without a null
    uint32_t tile0;         // its first tile
    uint32_t col;
    // OXH_PARQUET_DICTIONARY. A data page of a dictionary chunk: the chunk's index width (0: PLAIN values), its
    // dictionary page, and where its indices start in the call's dense index array (a multiple of 512). The dictionary
    // page itself (rows == 0, the chunk's first page): dict_page names it, nvalid = its entries, values_bytes its body.
    uint32_t dict_width, dict_page;
    uint64_t dense_at;
    // A list column's page (parquet_write_lists.hip). Its head is the PageHeader, the repetition stream's length and
    // run header; the definition stream's length and run header, def_head_len bytes, lie behind it in the blob and
    // behind the repetition bits in the file; level_bytes = the repetition bits + def_head_len + the definition bits;
    // nvalid = its values (the entries of definition level 3). entry0, value0: the page's first entry in the
    // column's entry space, and the values in front of it.
    uint64_t entry0, value0;
    uint32_t entries, def_head_len;
};

// What the rank step leaves per (row group, column), entry group * ncols + column.
struct ChunkDict {
    uint64_t num_values;   // the distinct values of the chunk's rows that are not null
    uint64_t dict_bytes;   // the dictionary page's body: 8 an entry, strings 4 + length
    uint64_t overflow;     // not 0: more than kDictMaxEntries values or a cell above kDictMaxCell; the other two words mean nothing
};

struct Place {
    uint32_t page;
    uint32_t rank_base;     // the valid rows of the page in front of the tile
    uint64_t byte_base;     // strings: their value bytes; booleans: the rank_base & 7 value bits of the page's earlier
                            // rows that share the tile's first byte, in the byte's order
};

#if defined(__HIPCC__)
#define OXH_PQ_BOTH __host__ __device__
#else
#define OXH_PQ_BOTH
#endif
// The values of the last 7 valid rows so far, the last one in bit 0, after 64 more rows (mask: not null, vals: the
// value bits of those). The measure kernel folds it over a tile's steps, the planner over a page's tiles.
OXH_PQ_BOTH inline uint32_t bool_tail(uint32_t tail, uint64_t mask, uint64_t vals) {
    uint32_t t = 0, cnt = 0;
    while (mask && cnt < 7) {
        const int j = 63 - __builtin_clzll(mask);
        mask &= ~(1ull << j);
        t |= (uint32_t)((vals >> j) & 1) << cnt;
        ++cnt;
    }
    return (t | (tail << cnt)) & 0x7F;
}

// ---------------------------------------------------------------- Thrift compact protocol
enum : uint8_t { kTBoolTrue = 1, kTBoolFalse = 2, kTI16 = 4, kTI32 = 5, kTI64 = 6, kTBinary = 8, kTList = 9, kTStruct = 12 };

struct Thrift {
    std::vector<uint8_t> out;
    std::vector<int16_t> last{0};  // the last field id of every open struct

    void varint(uint64_t v) {
        while (v >= 0x80) out.push_back((uint8_t)(v | 0x80)), v >>= 7;
        out.push_back((uint8_t)v);
    }
    static uint64_t zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
    void field(int16_t id, uint8_t type) {
        const int delta = id - last.back();
        if (delta > 0 && delta <= 15) {
            out.push_back((uint8_t)((delta << 4) | type));
        } else {
            out.push_back(type);
            varint(zigzag(id));
        }
        last.back() = id;
    }
    void i16(int16_t id, int16_t v) { field(id, kTI16), varint(zigzag(v)); }
    void i32(int16_t id, int32_t v) { field(id, kTI32), varint(zigzag(v)); }
    void i64(int16_t id, int64_t v) { field(id, kTI64), varint(zigzag(v)); }
    void raw_binary(const void* p, uint64_t n) {
        varint(n);
        out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n);
    }
    void binary(int16_t id, const void* p, uint64_t n) { field(id, kTBinary), raw_binary(p, n); }
    void list(int16_t id, uint8_t elem, uint64_t n) {
        field(id, kTList);
        if (n < 15) {
            out.push_back((uint8_t)((n << 4) | elem));
        } else {
            out.push_back((uint8_t)(0xF0 | elem));
            varint(n);
        }
    }
    void begin() { last.push_back(0); }                       // a struct that is a list element
    void begin(int16_t id) { field(id, kTStruct), begin(); }  // a struct that is a field
    void end() { out.push_back(0), last.pop_back(); }
};

OXH_PQ_BOTH inline uint32_t varint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) v >>= 7, ++n;
    return n;
}

// ---------------------------------------------------------------- arguments
struct Args {
    uint64_t nrows;
    uint32_t ncols;
    const uint32_t* types;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint8_t* names;
    const uint64_t* name_offsets;
    uint64_t rows_per_group, page_bytes;
    uint32_t flags;
    uint8_t* out;
    uint64_t capacity;
    uint64_t* out_bytes;
    uint64_t* stats4;
    const uint8_t* const* child_validity = nullptr;  // oxh_write_parquet_lists_*: the elements' bitmaps; NULL: none
    const uint64_t* child_bit_offsets = nullptr;     // per column the bit of element 0 in its child_validity
};

// A list column's type word: OXH_PARQUET_LIST on the element's word, with OXH_PARQUET_LIST64 for int64 offsets.
OXH_PQ_BOTH inline bool is_list(uint32_t t) { return (t & OXH_PARQUET_LIST) != 0; }
inline uint32_t list_element(uint32_t t) { return t & ~(uint32_t)(OXH_PARQUET_LIST | OXH_PARQUET_LIST64); }
inline bool list_element_known(uint32_t e) { return e == OXH_CSV_INT64 || e == OXH_CSV_FLOAT64 || e == OXH_CSV_INT32 || e == OXH_CSV_FLOAT32; }
inline uint32_t element_width(uint32_t t) { return list_element(t) == OXH_CSV_INT32 || list_element(t) == OXH_CSV_FLOAT32 ? 4 : 8; }
inline uint32_t list_offset_width(uint32_t t) { return t & OXH_PARQUET_LIST64 ? 8 : 4; }
inline bool dict_candidate(uint32_t t) { return !is_list(t) && t != OXH_CSV_BOOL; }  // OXH_PARQUET_DICTIONARY: a list chunk stays PLAIN

inline bool known_type(uint32_t t) { return t >= OXH_CSV_INT64 && t <= OXH_CSV_STRING64; }
inline bool is_string(uint32_t t) { return t == OXH_CSV_STRING || t == OXH_CSV_STRING64; }
inline uint32_t kind_of(uint32_t type) {
    if (is_list(type)) return element_width(type) == 4 ? OXH_COL_FIXED4 : OXH_COL_FIXED8;  // what its values table holds
    return type == OXH_CSV_BOOL ? OXH_COL_BOOL : type == OXH_CSV_STRING ? OXH_COL_BYTES32 : type == OXH_CSV_STRING64 ? OXH_COL_BYTES64 : OXH_COL_FIXED8;
}
inline uint64_t group_rows_of(uint64_t rows_per_group) { return rows_per_group ? rows_per_group : kDefaultGroupRows; }
inline uint64_t page_bytes_of(uint64_t page_bytes) { return page_bytes ? page_bytes : kDefaultPageBytes; }

inline bool bit_at(const uint8_t* p, uint64_t bit) { return (p[bit >> 3] >> (bit & 7)) & 1; }

// Host form: the elements [lo, hi) that the lists which are not null name; lo == hi when they name none. `bad_row`:
// the first list that is not null whose pair of offsets is negative or decreases (nrows: none).
struct ListSpan {
    uint64_t lo = 0, hi = 0, bad_row = 0;
};
inline ListSpan list_span(const Args& a, uint32_t c) {
    ListSpan s;
    s.bad_row = a.nrows;
    const bool wide = (a.types[c] & OXH_PARQUET_LIST64) != 0;
    bool any = false;
    for (uint64_t r = 0; r < a.nrows; ++r) {
        if (a.validity[c] && !bit_at(a.validity[c], a.bit_offsets[2 * c + 1] + r)) continue;
        const int64_t b = wide ? ((const int64_t*)a.offsets[c])[r] : ((const int32_t*)a.offsets[c])[r];
        const int64_t e = wide ? ((const int64_t*)a.offsets[c])[r + 1] : ((const int32_t*)a.offsets[c])[r + 1];
        if (b < 0 || e < b) return s.bad_row = r, s;
        if (e == b) continue;
        s.lo = any ? std::min<uint64_t>(s.lo, (uint64_t)b) : (uint64_t)b, s.hi = any ? std::max<uint64_t>(s.hi, (uint64_t)e) : (uint64_t)e;
        any = true;
    }
    return s;
}

// What is wrong with a list column of nrows > 0 rows: no offsets; offsets not aligned to their width; host (the offsets
// can be read): a list that is not null with a negative or decreasing pair, elements without values.
inline std::string list_error(const std::string& col, const Args& a, uint32_t c, bool host) {
    if (!a.offsets[c]) return col + " is a list column without offsets";
    const uint32_t ow = list_offset_width(a.types[c]);
    if ((uintptr_t)a.offsets[c] % ow) return col + ": list offsets are not aligned to " + std::to_string(ow) + " bytes";
    if (!host) return "";  // the offsets are on the device: the kernels check them
    const ListSpan s = list_span(a, c);
    if (s.bad_row < a.nrows) return col + ": list offsets decrease or are negative at row " + std::to_string(s.bad_row);
    if (!a.values[c] && s.hi > s.lo) return col + " has elements but no values";
    return "";
}

// "" when the arguments are well formed, else what is wrong with them, in the header's order.
inline std::string write_error(const Args& a, bool host) {
    if (!a.types || !a.kinds || !a.values || !a.offsets || !a.validity || !a.bit_offsets)
        return "types, kinds, values, offsets, validity or bit_offsets is NULL";
    if (a.ncols == 0) return "ncols is 0";
    if (a.flags & ~(kFlagSnappy | kFlagDictionary)) return "unknown flags";
    if (a.rows_per_group % kTileRows) return "rows_per_group is not a multiple of 1024";
    for (uint32_t c = 0; c < a.ncols; ++c) {
        if (is_list(a.types[c]) && !list_element_known(list_element(a.types[c])))
            return "column " + std::to_string(c) + " is a list of element type " + std::to_string(list_element(a.types[c])) + ": not int64, float64, int32 or float32";
        if (!is_list(a.types[c]) && !known_type(a.types[c])) return "column " + std::to_string(c) + " has unknown type " + std::to_string(a.types[c]);
    }
    for (uint32_t c = 0; c < a.ncols; ++c)
        if (a.kinds[c] != kind_of(a.types[c]))
            return "column " + std::to_string(c) + " of type " + std::to_string(a.types[c]) + " has kind " + std::to_string(a.kinds[c]) +
                   ", not " + std::to_string(kind_of(a.types[c]));
    if (!a.name_offsets) return "name_offsets is NULL";
    for (uint32_t c = 0; c < a.ncols; ++c)
        if (a.name_offsets[c + 1] < a.name_offsets[c]) return "name_offsets decrease at column " + std::to_string(c);
    if (!a.names && a.name_offsets[a.ncols] > a.name_offsets[0]) return "names is NULL";
    if (!a.out_bytes || !a.stats4) return "out_bytes or stats4 is NULL";
    if (a.nrows > kMaxRows) return "more than 2^40 rows";
    for (uint32_t c = 0; c < a.ncols && a.nrows; ++c) {
        const std::string col = "column " + std::to_string(c);
        const std::string what = is_list(a.types[c]) ? list_error(col, a, c, host) : oxh::cols::column_error(col, a.kinds[c], a.values[c], a.offsets[c], a.nrows, host);
        if (!what.empty()) return what;
    }
    return "";
}

// ---------------------------------------------------------------- statistics
// A column chunk's min / max from its tiles' partials. DOUBLE follows the format's rule: the NaNs were left out by
// the kernel, no value at all gives no min / max, a min of zero is -0.0 and a max of zero is +0.0.
struct MinMax {
    bool has = false;
    uint64_t min = 0, max = 0;
    static double as_double(uint64_t bits) {
        double d;
        memcpy(&d, &bits, 8);
        return d;
    }
    void fold(const Tile& t, uint32_t type) {
        if (!t.has_minmax) return;
        if (!has) {
            has = true, min = t.min, max = t.max;
        } else if (type == OXH_CSV_INT64) {
            if ((int64_t)t.min < (int64_t)min) min = t.min;
            if ((int64_t)t.max > (int64_t)max) max = t.max;
        } else {
            if (as_double(t.min) < as_double(min)) min = t.min;
            if (as_double(t.max) > as_double(max)) max = t.max;
        }
    }
    void finish(uint32_t type) {
        if (!has || type != OXH_CSV_FLOAT64) return;
        if (as_double(min) == 0.0) min = 0x8000000000000000ull;
        if (as_double(max) == 0.0) max = 0;
    }
};

// ---------------------------------------------------------------- the plan
struct Plan {
    std::vector<Page> pages;
    std::vector<Place> places;     // ntiles * ncols
    std::vector<uint8_t> blob;     // the pages' heads, one after the other
    std::vector<uint32_t> header_len;  // per page: the bytes of its PageHeader, the front of its head; the body starts behind
    std::vector<uint8_t> footer;   // FileMetaData, its u32 length, "PAR1"
    uint64_t out_bytes = 0, row_groups = 0, null_cells = 0;
    uint64_t stored_bytes = 0, plain_bytes = 0;  // the row groups' total_compressed_size and total_byte_size, summed
    uint64_t dense_indices = 0;    // OXH_PARQUET_DICTIONARY: the dense index array's u32 words
    std::string error;             // not empty: the file is refused
};

// Bytes of a page of `rows` rows: its levels (with their u32 length) and its values.
inline uint64_t level_run_len(uint64_t rows, bool nulls) {
    return nulls ? varint_len((((rows + 7) / 8) << 1) | 1) + (rows + 7) / 8 : varint_len(rows << 1) + 1;
}
inline uint64_t values_len(uint32_t type, uint64_t valid, uint64_t bytes) { return type == OXH_CSV_BOOL ? (valid + 7) / 8 : bytes; }

// OXH_PARQUET_DICTIONARY: whether a chunk is written with a dictionary (the three limits of the header; a chunk without
// a value has none), the width of its indices, and the bytes of a page's index stream: the width byte, then one
// bit-packed run of ceil(valid / 8) groups -- nothing behind the width for a page without a valid row.
inline bool dict_chunk(uint32_t type, const ChunkDict& d) {
    return dict_candidate(type) && !d.overflow && d.num_values >= 1 && d.num_values <= kDictMaxEntries && d.dict_bytes <= kDictMaxPage;
}
inline uint32_t dict_width(uint64_t num_values) {
    uint32_t w = 1;
    while ((1ull << w) < num_values) ++w;
    return w;
}
inline uint64_t index_stream_len(uint64_t valid, uint32_t w) {
    const uint64_t groups = (valid + 7) / 8;
    return groups ? 1 + varint_len((groups << 1) | 1) + groups * w : 1;
}
constexpr uint64_t kDenseBlock = 512;  // the indices one wave packs; a page's place in the dense array is a multiple of it

inline void put_u32(std::vector<uint8_t>& out, uint32_t v) {
    for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(v >> (8 * k)));
}

// ---------------------------------------------------------------- a list page's level streams
// One stream of n >= 1 entries at `width` bits is one run of the hybrid. RLE (every entry is `value`): varint(n << 1)
// and the value's byte. Bit-packed: varint((ceil(n / 8) << 1) | 1), then ceil(n / 8) * width bytes, LSB first, the
// pad entries 0. Which form depends on counts alone: repetition (width 1) is RLE of 0 when the page's entries equal
// its rows, definition (width 2) RLE of 3 when its values equal its entries.
inline uint64_t level_packed_bytes(uint64_t n, uint32_t width, bool rle) { return rle ? 0 : (n + 7) / 8 * width; }
inline uint64_t level_stream_len(uint64_t n, uint32_t width, bool rle) {
    return rle ? varint_len(n << 1) + 1 : varint_len((((n + 7) / 8) << 1) | 1) + level_packed_bytes(n, width, false);
}
// The stream's head as the page carries it: the run's u32 length, its header and, for RLE, the value byte. The
// packed bytes behind a bit-packed head are the emit kernel's.
inline void put_level_head(Thrift& th, uint64_t n, uint32_t width, bool rle, uint8_t value) {
    put_u32(th.out, (uint32_t)level_stream_len(n, width, rle));
    if (rle) {
        th.varint(n << 1);
        th.out.push_back(value);
    } else {
        th.varint((((n + 7) / 8) << 1) | 1);
    }
}
// Bytes of a list page's body: both streams with their lengths, then the PLAIN values.
inline uint64_t list_body_len(uint64_t rows, uint64_t entries, uint64_t values, uint32_t width) {
    return 8 + level_stream_len(entries, 1, entries == rows) + level_stream_len(entries, 2, values == entries) + values * width;
}

struct ChunkMeta {
    uint64_t first_page_at = 0, dict_page_at = 0, bytes = 0, plain_bytes = 0, rows = 0, nulls = 0;  // bytes: as stored; plain_bytes: uncompressed
    MinMax mm;
    bool dict = false;
};

inline int32_t parquet_type(uint32_t t) {
    if (is_list(t)) return list_element(t) == OXH_CSV_INT64 ? 2 : list_element(t) == OXH_CSV_FLOAT64 ? 5 : list_element(t) == OXH_CSV_INT32 ? 1 : 4;
    return t == OXH_CSV_INT64 ? 2 : t == OXH_CSV_FLOAT64 ? 5 : t == OXH_CSV_BOOL ? 0 : 6;
}

// One page of a list column's chunk from tile t on (t < t1 afterwards): whole tiles until both level streams and the
// values reach the budget. A list column's tile: min = its level entries, value_bytes = its values' bytes, valid = its
// lists that are not null. pg comes with file_at, row0, tile0 and col set; false: p.error says why the file is refused.
inline bool plan_list_page(Plan& p, Page pg, ChunkMeta& m, uint64_t& at, uint64_t& t, uint64_t t1, uint64_t nrows, uint32_t ncols, uint32_t c,
                           uint32_t type, const Tile* tiles, const uint64_t* stored, uint64_t budget, uint64_t& entry_at, uint64_t& value_at) {
    const uint32_t w = element_width(type);
    uint64_t rows = 0, valid = 0, bytes = 0, entries = 0;
    do {
        const Tile& tl = tiles[t * ncols + c];
        const uint64_t tile_rows = std::min(nrows - t * kTileRows, kTileRows);
        if (tl.valid > tile_rows || tl.min < tile_rows || tl.value_bytes % w || tl.value_bytes / w > tl.min)
            return p.error = "a tile of a list column counts what it cannot hold", false;
        p.places[t * ncols + c] = Place{(uint32_t)p.pages.size(), 0, 0};
        rows += tile_rows, valid += tl.valid, bytes += tl.value_bytes, entries += tl.min;
        ++t;
    } while (t < t1 && list_body_len(rows, entries, bytes / w, w) < budget);
    const uint64_t values = bytes / w, body = list_body_len(rows, entries, values, w);
    if (body > kMaxPage || entries > kMaxPage)
        return p.error = "a page of column " + std::to_string(c) + " has " + std::to_string(body) + " B and " + std::to_string(entries) +
                         " level entries: more than a PageHeader's int32", false;
    const uint64_t kept = stored ? stored[p.pages.size()] : body;
    if (kept > kMaxPage) return p.error = "a compressed page of column " + std::to_string(c) + " has more than a PageHeader's int32", false;
    Thrift th;
    th.i32(1, 0);  // DATA_PAGE
    th.i32(2, (int32_t)body), th.i32(3, (int32_t)kept);
    th.begin(5);
    th.i32(1, (int32_t)entries), th.i32(2, 0), th.i32(3, 3), th.i32(4, 3);  // num_values counts entries; PLAIN, RLE, RLE
    th.end();
    th.out.push_back(0);
    p.header_len.push_back((uint32_t)th.out.size());
    const bool rep_rle = entries == rows, def_rle = values == entries;
    put_level_head(th, entries, 1, rep_rle, 0);
    pg.head_src = p.blob.size(), pg.head_len = (uint32_t)th.out.size();
    put_level_head(th, entries, 2, def_rle, 3);
    pg.def_head_len = (uint32_t)th.out.size() - pg.head_len;
    pg.level_bytes = (uint32_t)(level_packed_bytes(entries, 1, rep_rle) + pg.def_head_len + level_packed_bytes(entries, 2, def_rle));
    pg.values_bytes = bytes, pg.rows = (uint32_t)rows, pg.nvalid = (uint32_t)values, pg.entries = (uint32_t)entries;
    pg.entry0 = entry_at, pg.value0 = value_at;
    entry_at += entries, value_at += values;
    p.blob.insert(p.blob.end(), th.out.begin(), th.out.end());
    const uint64_t plain_whole = p.header_len.back() + body;
    const uint64_t whole = stored ? p.header_len.back() + kept : plain_whole;
    if (stored) pg.values_bytes = kept;
    at += whole, m.bytes += whole, m.plain_bytes += plain_whole, m.rows += entries, m.nulls += rows - valid;
    p.pages.push_back(pg);
    return true;
}

// tiles: ceil(nrows / 1024) * ncols entries. The names are read as write_error() left them.
// stored: NULL for an uncompressed file; else the plan of the SNAPPY file whose page k's body is stored in stored[k]
// bytes (the pages in this function's own order: the same cuts as the uncompressed plan's, whose page_bytes counts
// uncompressed bytes). Such a plan's pages name where the header goes (file_at, head_src, header_len) and how long
// the stored body is (values_bytes); its chunks are codec SNAPPY, total_compressed_size the stored bytes and
// total_uncompressed_size the headers as written plus the uncompressed bodies, the format's rule.
// dicts: NULL without OXH_PARQUET_DICTIONARY; else ceil(nrows / group rows) * ncols entries. A chunk that dict_chunk()
// accepts starts with its dictionary page -- one more entry of `pages` (and of `stored`), in the file's order -- and its
// data pages are RLE_DICTIONARY, cut by the index stream's bytes; every other chunk is what it is without the flag.
inline Plan make_plan(uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint8_t* names, const uint64_t* name_offsets,
                      uint64_t rows_per_group, uint64_t page_bytes, const Tile* tiles, const uint64_t* stored = nullptr,
                      const ChunkDict* dicts = nullptr) {
    Plan p;
    const uint64_t group_rows = group_rows_of(rows_per_group), budget = page_bytes_of(page_bytes);
    const uint64_t ntiles = (nrows + kTileRows - 1) / kTileRows, group_tiles = group_rows / kTileRows;
    p.places.resize(ntiles * ncols);
    uint64_t at = 4;  // behind "PAR1"
    struct Group {
        uint64_t rows, at, bytes, plain_bytes;
        std::vector<ChunkMeta> chunks;
    };
    std::vector<Group> groups;
    std::vector<uint64_t> entry_at(ncols, 0), value_at(ncols, 0);  // list columns: the entries and values of the pages so far
    for (uint64_t t0 = 0; t0 < ntiles; t0 += group_tiles) {
        const uint64_t t1 = std::min(ntiles, t0 + group_tiles);
        Group g{std::min(nrows, t1 * kTileRows) - t0 * kTileRows, at, 0, 0, std::vector<ChunkMeta>(ncols)};
        for (uint32_t c = 0; c < ncols; ++c) {
            ChunkMeta& m = g.chunks[c];
            m.dict = dicts && dict_chunk(types[c], dicts[groups.size() * ncols + c]);
            const uint32_t width = m.dict ? dict_width(dicts[groups.size() * ncols + c].num_values) : 0;
            const uint32_t dict_page = (uint32_t)p.pages.size();
            const auto values_of = [&](uint64_t valid, uint64_t bytes) { return m.dict ? index_stream_len(valid, width) : values_len(types[c], valid, bytes); };
            if (m.dict) {  // the dictionary page: its header, the entries behind it
                const ChunkDict& d = dicts[groups.size() * ncols + c];
                Page pg{};
                pg.file_at = m.dict_page_at = at, pg.row0 = t0 * kTileRows, pg.tile0 = (uint32_t)t0, pg.col = c;
                pg.nvalid = (uint32_t)d.num_values, pg.dict_width = width, pg.dict_page = dict_page;
                const uint64_t kept = stored ? stored[p.pages.size()] : d.dict_bytes;
                if (kept > kMaxPage) return p.error = "a compressed page of column " + std::to_string(c) + " has more than a PageHeader's int32", p;
                Thrift th;
                th.i32(1, 2);  // DICTIONARY_PAGE
                th.i32(2, (int32_t)d.dict_bytes), th.i32(3, (int32_t)kept);
                th.begin(7);
                th.i32(1, (int32_t)d.num_values), th.i32(2, 0);  // PLAIN
                th.end();
                th.out.push_back(0);
                p.header_len.push_back((uint32_t)th.out.size());
                pg.head_src = p.blob.size(), pg.head_len = (uint32_t)th.out.size(), pg.values_bytes = kept;
                p.blob.insert(p.blob.end(), th.out.begin(), th.out.end());
                at += pg.head_len + kept, m.bytes += pg.head_len + kept, m.plain_bytes += pg.head_len + d.dict_bytes;
                p.pages.push_back(pg);
            }
            m.first_page_at = at;
            for (uint64_t t = t0; t < t1;) {
                // one page: whole tiles until the levels and the values reach the budget
                Page pg{};
                pg.file_at = at, pg.row0 = t * kTileRows, pg.tile0 = (uint32_t)t, pg.col = c;
                uint64_t rows = 0, valid = 0, bytes = 0;
                uint32_t carry = 0;  // booleans: bool_tail of the page so far
                if (is_list(types[c])) {
                    if (!plan_list_page(p, pg, m, at, t, t1, nrows, ncols, c, types[c], tiles, stored, budget, entry_at[c], value_at[c])) return p;
                    continue;
                }
                do {
                    const Tile& tl = tiles[t * ncols + c];
                    const uint64_t tile_rows = std::min(nrows - t * kTileRows, kTileRows);
                    if (tl.valid > tile_rows) return p.error = "a tile counts more valid rows than it has", p;
                    uint64_t lead = 0;  // the carry's newest valid & 7 bits, the oldest of them in bit 0
                    for (uint32_t k = 0; k < (valid & 7); ++k) lead |= (uint64_t)((carry >> ((valid & 7) - 1 - k)) & 1) << k;
                    p.places[t * ncols + c] = Place{(uint32_t)p.pages.size(), (uint32_t)valid, types[c] == OXH_CSV_BOOL ? lead : bytes};
                    if (types[c] == OXH_CSV_BOOL) {
                        const uint32_t cnt = std::min<uint32_t>(tl.valid, 7);
                        carry = (((uint32_t)tl.min & ((1u << cnt) - 1)) | (carry << cnt)) & 0x7F;
                    }
                    rows += tile_rows, valid += tl.valid, bytes += tl.value_bytes;
                    m.mm.fold(tl, types[c]);
                    ++t;
                } while (t < t1 && 4 + level_run_len(rows, valid < rows) + values_of(valid, bytes) < budget);
                const bool nulls = valid < rows;
                const uint64_t run = level_run_len(rows, nulls), vbytes = values_of(valid, bytes);
                const uint64_t body = 4 + run + vbytes;
                if (body > kMaxPage || rows > kMaxPage)
                    return p.error = "a page of column " + std::to_string(c) + " has " + std::to_string(body) + " B: more than a PageHeader's int32", p;
                Thrift th;
                th.i32(1, 0);  // DATA_PAGE
                const uint64_t kept = stored ? stored[p.pages.size()] : body;
                if (kept > kMaxPage) return p.error = "a compressed page of column " + std::to_string(c) + " has more than a PageHeader's int32", p;
                th.i32(2, (int32_t)body), th.i32(3, (int32_t)kept);
                th.begin(5);
                th.i32(1, (int32_t)rows), th.i32(2, m.dict ? 8 : 0), th.i32(3, 3), th.i32(4, 3);  // PLAIN or RLE_DICTIONARY, RLE, RLE
                th.end();
                th.out.push_back(0);
                p.header_len.push_back((uint32_t)th.out.size());
                put_u32(th.out, (uint32_t)run);
                if (nulls) {
                    th.varint((((rows + 7) / 8) << 1) | 1);
                } else {
                    th.varint(rows << 1);
                    th.out.push_back(1);
                }
                pg.head_src = p.blob.size(), pg.head_len = (uint32_t)th.out.size();
                pg.level_bytes = nulls ? (uint32_t)((rows + 7) / 8) : 0;
                pg.values_bytes = vbytes, pg.rows = (uint32_t)rows, pg.nvalid = (uint32_t)valid;
                if (m.dict) {
                    pg.dict_width = width, pg.dict_page = dict_page, pg.dense_at = p.dense_indices;
                    p.dense_indices += (valid + kDenseBlock - 1) / kDenseBlock * kDenseBlock;
                }
                p.blob.insert(p.blob.end(), th.out.begin(), th.out.end());
                const uint64_t plain_whole = pg.head_len + pg.level_bytes + vbytes;  // == the header's bytes + body
                const uint64_t whole = stored ? p.header_len.back() + kept : plain_whole;
                if (stored) pg.values_bytes = kept;
                at += whole, m.bytes += whole, m.plain_bytes += plain_whole, m.rows += rows, m.nulls += rows - valid;
                p.pages.push_back(pg);
            }
            m.mm.finish(types[c]);
            g.bytes += m.bytes, g.plain_bytes += m.plain_bytes, p.null_cells += m.nulls;
        }
        groups.push_back(std::move(g));
    }
    if (groups.size() > 32767) return p.error = std::to_string(groups.size()) + " row groups: more than a RowGroup's int16 ordinal", p;
    // the footer
    Thrift f;
    f.i32(1, 1);
    uint32_t nlists = 0;
    for (uint32_t c = 0; c < ncols; ++c) nlists += is_list(types[c]);
    f.list(2, kTStruct, ncols + 1 + 2ull * nlists);
    f.begin();
    f.i32(3, 0), f.binary(4, "schema", 6), f.i32(5, (int32_t)ncols);
    f.end();
    for (uint32_t c = 0; c < ncols; ++c) {
        if (is_list(types[c])) {  // OPTIONAL group <name> (LIST) { REPEATED group list { OPTIONAL <T> element } }
            f.begin();
            f.i32(3, 1), f.binary(4, names + name_offsets[c], name_offsets[c + 1] - name_offsets[c]), f.i32(5, 1), f.i32(6, 3);  // converted type LIST
            f.begin(10), f.begin(3), f.end(), f.end();  // LogicalType.LIST
            f.end();
            f.begin();
            f.i32(3, 2), f.binary(4, "list", 4), f.i32(5, 1);  // REPEATED
            f.end();
            f.begin();
            f.i32(1, parquet_type(types[c])), f.i32(3, 1), f.binary(4, "element", 7);
            f.end();
            continue;
        }
        f.begin();
        f.i32(1, parquet_type(types[c])), f.i32(3, 1);  // OPTIONAL
        f.binary(4, names + name_offsets[c], name_offsets[c + 1] - name_offsets[c]);
        if (is_string(types[c])) {
            f.i32(6, 0);  // UTF8
            f.begin(10), f.begin(1), f.end(), f.end();  // LogicalType.STRING
        }
        f.end();
    }
    f.i64(3, (int64_t)nrows);
    f.list(4, kTStruct, groups.size());
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& g = groups[gi];
        f.begin();
        f.list(1, kTStruct, ncols);
        for (uint32_t c = 0; c < ncols; ++c) {
            const ChunkMeta& m = g.chunks[c];
            f.begin();
            f.i64(2, 0);  // file_offset: unused since the metadata sits in the footer
            f.begin(3);
            f.i32(1, parquet_type(types[c]));
            f.list(2, kTI32, m.dict ? 3 : 2), f.varint(Thrift::zigzag(0)), f.varint(Thrift::zigzag(3));  // PLAIN, RLE
            if (m.dict) f.varint(Thrift::zigzag(8));  // RLE_DICTIONARY
            f.list(3, kTBinary, is_list(types[c]) ? 3 : 1), f.raw_binary(names + name_offsets[c], name_offsets[c + 1] - name_offsets[c]);
            if (is_list(types[c])) f.raw_binary("list", 4), f.raw_binary("element", 7);
            f.i32(4, stored ? 1 : 0);  // SNAPPY, UNCOMPRESSED
            f.i64(5, (int64_t)m.rows), f.i64(6, (int64_t)m.plain_bytes), f.i64(7, (int64_t)m.bytes);  // num_values: a list chunk's entries
            f.i64(9, (int64_t)m.first_page_at);
            if (m.dict) f.i64(11, (int64_t)m.dict_page_at);
            if (!is_list(types[c])) {  // a list chunk has no statistics
                f.begin(12);
                f.i64(3, (int64_t)m.nulls);
                if (m.mm.has) f.binary(5, &m.mm.max, 8), f.binary(6, &m.mm.min, 8);
                f.end();
            }
            f.end();
            f.end();
        }
        f.i64(2, (int64_t)g.plain_bytes), f.i64(3, (int64_t)g.rows), f.i64(5, (int64_t)g.at), f.i64(6, (int64_t)g.bytes);
        f.i16(7, (int16_t)gi);
        f.end();
    }
    f.binary(6, kCreatedBy, strlen(kCreatedBy));
    f.list(7, kTStruct, ncols);
    for (uint32_t c = 0; c < ncols; ++c) f.begin(), f.begin(1), f.end(), f.end();  // ColumnOrder.TYPE_ORDER
    f.out.push_back(0);
    p.footer = std::move(f.out);
    const uint64_t meta = p.footer.size();
    if (meta > 0xFFFFFFFFull) return p.error = "the footer has " + std::to_string(meta) + " B: more than its u32 length", p;
    put_u32(p.footer, (uint32_t)meta);
    p.footer.insert(p.footer.end(), {'P', 'A', 'R', '1'});
    p.row_groups = groups.size();
    for (const Group& g : groups) p.stored_bytes += g.bytes, p.plain_bytes += g.plain_bytes;
    p.out_bytes = at + p.footer.size();
    return p;
}

// A capacity that holds the SNAPPY file of an uncompressed plan whatever its pages hold: every body at Snappy's
// bound (32 + n + n / 6), every PageHeader with a 5-byte compressed size, and 10 bytes more for each of the footer's
// sizes and offsets (5 a chunk, 4 a row group), which can only grow where pages do.
inline uint64_t snappy_capacity(const Plan& plain, uint32_t ncols) {
    uint64_t bytes = plain.out_bytes + 10 * plain.row_groups * (5ull * ncols + 4);
    for (size_t k = 0; k < plain.pages.size(); ++k) {
        const Page& pg = plain.pages[k];
        const uint64_t body = pg.head_len - plain.header_len[k] + pg.level_bytes + pg.values_bytes;
        bytes += 32 + body / 6 + 5;
    }
    return bytes;
}

}  // namespace oxh::parquet
