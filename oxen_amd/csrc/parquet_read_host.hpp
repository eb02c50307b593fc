// oxen_amd/csrc/parquet_read_host.hpp -- the host-only pieces of oxh_parquet_* (parquet_read.hip): the argument
// checks in the header's order; the footer (a Thrift compact FileMetaData, read through parquet_bits.hpp) turned into
// a plan -- the schema's leaves and, per row group and column, where the chunk's first page starts, its bytes, its
// num_values and its codec -- with every offset and size checked against the file before anything is launched; and
// the checks of the page table the walk kernel leaves, which turn it into the per-column page lists the column
// kernels read. Plain C++ with no HIP in it, so that a stand-alone program can call it
// (tests/native/parquet_read_host_test.cpp, which is also what a sanitizer build runs).
#pragma once

#include <string.h>

#include <string>
#include <vector>

#include "csv_host.hpp"
#include "parquet_bits.hpp"

namespace oxh::pqr {

constexpr uint64_t kMaxRows = 1ull << 40;
constexpr uint64_t kMaxPage = 0x7FFFFFFFull;
enum : int32_t { kBoolean = 0, kInt32 = 1, kInt64 = 2, kInt96 = 3, kFloat = 4, kDouble = 5, kByteArray = 6, kFixedLen = 7 };

inline const char* physical_name(int32_t t) {
    static const char* names[] = {"BOOLEAN", "INT32", "INT64", "INT96", "FLOAT", "DOUBLE", "BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY"};
    return t >= 0 && t <= 7 ? names[t] : "an unknown physical type";
}
// The type word a column of this physical type is read as when the caller names none (0: this reader has none).
inline uint32_t native_type(int32_t physical) {
    switch (physical) {
        case kBoolean: return OXH_CSV_BOOL;
        case kInt32: return OXH_CSV_INT32;
        case kInt64: return OXH_CSV_INT64;
        case kFloat: return OXH_CSV_FLOAT32;
        case kDouble: return OXH_CSV_FLOAT64;
        case kByteArray: return OXH_CSV_STRING;
        default: return 0;
    }
}
inline bool type_fits(int32_t physical, uint32_t type) {
    if (type == native_type(physical)) return type != 0;
    return (physical == kInt32 && type == OXH_CSV_INT64) || (physical == kFloat && type == OXH_CSV_FLOAT64) ||
           (physical == kByteArray && type == OXH_CSV_STRING64);
}
// A list column's type word: OXH_PARQUET_LIST, with or without OXH_PARQUET_LIST64, on its element's word.
constexpr uint32_t kListBits = OXH_PARQUET_LIST | OXH_PARQUET_LIST64;
inline bool is_list_word(uint32_t type) { return (type & OXH_PARQUET_LIST) && !(type & ~(kListBits | 7u)); }
inline uint32_t element_word(uint32_t type) { return type & ~kListBits; }
inline bool list_element_read(int32_t physical) { return physical == kInt32 || physical == kInt64 || physical == kFloat || physical == kDouble; }

struct Leaf {
    std::string name;
    int32_t physical = -1;
    bool required = false;
    std::string cause;  // not empty: why this reader cannot read the column
    // A three-level LIST directly under the root: the leaf is its element, `name` and `required` are the list's.
    // An entry of definition level d: d >= def_list, the row's list is not null; d >= def_slot, an element is there,
    // null or not; d == max_def, it has a value. Max repetition level 1.
    bool list = false;
    uint32_t def_list = 0, def_slot = 0, max_def = 0;
};
// Bits of a level of at most `max` (the format's bit_width).
inline uint32_t level_width(uint32_t max) {
    uint32_t w = 0;
    while (max >> w) ++w;
    return w;
}

struct Chunk {
    uint64_t at = 0, bytes = 0, num_values = 0;
    uint32_t codec = 0;  // kCodecNone, or with OXH_PARQUET_INFLATE kCodecSnappy, with OXH_PARQUET_INFLATE_ZSTD kCodecZstd
};
constexpr uint32_t kCodecNone = 0, kCodecSnappy = 1, kCodecZstd = 6;

// No Snappy stream expands more than 64 / 3 (a 3-byte copy gives 64 bytes); the preamble and a short last element
// are the 32. A page that claims more is refused before anything is allocated for it.
inline bool inflated_size_plausible(uint64_t csize, uint64_t usize) { return usize <= 22 * csize + 32; }
// A Zstandard frame is a header of at least 5 bytes (the magic and the descriptor) and blocks that each cost at least
// 3 bytes (the block header) and yield at most 128 KiB: an RLE block of 4 bytes gives that much, so Snappy's bound
// is wrong here.
inline bool zstd_size_plausible(uint64_t csize, uint64_t usize) { return csize >= 5 && usize <= (csize - 5) / 3 * 131072; }

struct Footer {
    std::vector<Leaf> leaves;
    std::vector<uint64_t> group_rows;
    std::vector<Chunk> chunks;  // group * ncols + column
    uint64_t nrows = 0, footer_bytes = 0;
    std::string error;          // not empty: the file is refused
};

// "" when oxh_parquet_open_*'s arguments are well formed.
inline std::string open_error(const uint8_t* bytes, uint64_t nbytes, uint32_t flags, void* const* out, const uint64_t* stats8) {
    if (flags & ~(uint32_t)(OXH_PARQUET_INFLATE | OXH_PARQUET_INFLATE_ZSTD)) return "unknown flags";
    if (nbytes && !bytes) return "bytes is NULL";
    if (!out) return "out is NULL";
    if (!stats8) return "stats8 is NULL";
    return "";
}

// Where the footer is: "" and [at, at + len) of the file, or the refusal. tail: the file's last 8 bytes; head: its
// first 4.
inline std::string footer_place(const uint8_t* head, const uint8_t* tail, uint64_t nbytes, uint64_t& at, uint64_t& len) {
    if (nbytes < 12) return "a file of " + std::to_string(nbytes) + " bytes (the magics and the footer's length take 12)";
    if (!memcmp(tail + 4, "PARE", 4) || !memcmp(head, "PARE", 4)) return "an encrypted file (magic PARE)";
    if (memcmp(tail + 4, "PAR1", 4)) return "the file does not end with the magic PAR1";
    if (memcmp(head, "PAR1", 4)) return "the file does not start with the magic PAR1";
    len = le32(tail);
    if (len > nbytes - 12) return "a footer of " + std::to_string(len) + " bytes in a file of " + std::to_string(nbytes);
    at = nbytes - 8 - len;
    return "";
}

namespace detail {

struct Element {
    std::string name;
    int32_t type = -1, repetition = 0, children = -1;
    bool is_list = false;  // converted type LIST (3) or logical type LIST (the union's field 3)
};

inline std::string binary(Span& s) {
    const uint64_t n = varint(s);
    if (s.bad || n > s.n - s.at) return s.bad = true, std::string();
    std::string out((const char*)s.p + s.at, n);
    s.at += n;
    return out;
}

inline Element schema_element(Span& s) {
    Element e;
    uint64_t st[kSkipDepth];
    int32_t last = 0, id;
    uint32_t type;
    while (next_field(s, last, id, type)) {
        if (id == 1 && type == kTI32)
            e.type = i32_field(s);
        else if (id == 3 && type == kTI32)
            e.repetition = i32_field(s);
        else if (id == 4 && type == kTBinary)
            e.name = binary(s);
        else if (id == 5 && type == kTI32)
            e.children = i32_field(s);
        else if (id == 6 && type == kTI32)
            e.is_list |= i32_field(s) == 3;
        else if (id == 10 && type == kTStruct) {
            int32_t l2 = 0, i2;
            uint32_t t2;
            while (next_field(s, l2, i2, t2)) {
                e.is_list |= i2 == 3;
                if (t2 != kTTrue && t2 != kTFalse) skip_value(s, t2, st);
            }
        } else if (type != kTTrue && type != kTFalse)
            skip_value(s, type, st);
    }
    return e;
}

struct ChunkMeta {
    int64_t codec = 0, num_values = -1, compressed = -1, data_at = -1, dict_at = -1;
    bool has_meta = false, encrypted = false;
};

inline ChunkMeta column_chunk(Span& s) {
    ChunkMeta m;
    uint64_t st[kSkipDepth];
    int32_t last = 0, id;
    uint32_t type;
    while (next_field(s, last, id, type)) {
        if (id == 3 && type == kTStruct) {
            m.has_meta = true;
            int32_t l2 = 0, i2;
            uint32_t t2;
            while (next_field(s, l2, i2, t2)) {
                if (i2 == 4 && t2 == kTI32)
                    m.codec = zint(s);
                else if (i2 == 5 && t2 == kTI64)
                    m.num_values = zint(s);
                else if (i2 == 7 && t2 == kTI64)
                    m.compressed = zint(s);
                else if (i2 == 9 && t2 == kTI64)
                    m.data_at = zint(s);
                else if (i2 == 11 && t2 == kTI64)
                    m.dict_at = zint(s);
                else if (t2 != kTTrue && t2 != kTFalse)
                    skip_value(s, t2, st);
            }
        } else {
            if (id == 8 || id == 9) m.encrypted = true;  // crypto_metadata, encrypted_column_metadata
            if (type != kTTrue && type != kTFalse) skip_value(s, type, st);
        }
    }
    return m;
}

}  // namespace detail

// The plan of the file whose footer is the `len` bytes at `meta`, themselves at `meta_at` of the nbytes of the file.
// Refusals, in this order: a footer that is no FileMetaData; an encrypted footer; a schema without a root or whose
// elements are not the root's children (a nested field, named -- a three-level LIST of one leaf is a column, see
// Leaf); a repeated field; more than 2^40 rows; and per
// row group, in order: a column count that is not the schema's, a chunk without metadata or with encrypted
// metadata, a codec other than UNCOMPRESSED -- with `inflate` (OXH_PARQUET_INFLATE) other than that and SNAPPY, with
// `zstd` (OXH_PARQUET_INFLATE_ZSTD) and ZSTD -- (its number named), a chunk outside the file's pages, a num_values that is not the group's rows (a list's chunk: less than them); then group rows that do
// not sum to num_rows.
inline Footer read_footer(const uint8_t* meta, uint64_t len, uint64_t meta_at, uint64_t nbytes, bool inflate = false, bool zstd = false) {
    using namespace detail;
    Footer f;
    uint64_t st[kSkipDepth];
    f.footer_bytes = len;
    Span s{meta, len, 0, false};
    std::vector<Element> elements;
    std::vector<std::vector<ChunkMeta>> groups;
    std::vector<int64_t> group_rows;
    int64_t num_rows = -1;
    bool encrypted = false, has_schema = false;
    int32_t last = 0, id;
    uint32_t type;
    while (next_field(s, last, id, type)) {
        if (id == 2 && type == kTList) {
            uint32_t elem;
            uint64_t count;
            list_header(s, elem, count);
            if (elem != kTStruct) s.bad = true;
            has_schema = true;
            for (uint64_t k = 0; k < count && !s.bad; ++k) elements.push_back(schema_element(s));
        } else if (id == 3 && type == kTI64) {
            num_rows = zint(s);
        } else if (id == 4 && type == kTList) {
            uint32_t elem;
            uint64_t count;
            list_header(s, elem, count);
            if (elem != kTStruct) s.bad = true;
            for (uint64_t g = 0; g < count && !s.bad; ++g) {
                groups.emplace_back();
                group_rows.push_back(-1);
                int32_t l2 = 0, i2;
                uint32_t t2;
                while (next_field(s, l2, i2, t2)) {
                    if (i2 == 1 && t2 == kTList) {
                        uint32_t e2;
                        uint64_t c2;
                        list_header(s, e2, c2);
                        if (e2 != kTStruct) s.bad = true;
                        for (uint64_t c = 0; c < c2 && !s.bad; ++c) groups.back().push_back(column_chunk(s));
                    } else if (i2 == 3 && t2 == kTI64) {
                        group_rows.back() = zint(s);
                    } else if (t2 != kTTrue && t2 != kTFalse) {
                        skip_value(s, t2, st);
                    }
                }
            }
        } else {
            if (id == 8 || id == 9) encrypted = true;  // encryption_algorithm, footer_signing_key_metadata
            if (type != kTTrue && type != kTFalse) skip_value(s, type, st);
        }
    }
    if (s.bad || !has_schema || num_rows < 0) return f.error = "the footer is not a FileMetaData (Thrift compact) with a schema and num_rows", f;
    if (encrypted) return f.error = "an encrypted file (the footer names an encryption algorithm)", f;
    if (elements.empty() || elements[0].children < 0) return f.error = "the schema has no root group", f;
    // The root's children in order: a leaf, or the three elements of a LIST (group, REPEATED group, leaf). Any other
    // group stops the file, whether or not the root's count fits.
    uint64_t children = 0;
    for (size_t k = 1; k < elements.size(); ++children) {
        const Element& e = elements[k];
        if (e.children > 0) {
            const bool shaped = e.is_list && e.repetition != 2 && e.children == 1 && k + 2 < elements.size() && elements[k + 1].repetition == 2 &&
                                elements[k + 1].children == 1 && elements[k + 2].children <= 0 && elements[k + 2].repetition != 2;
            if (!shaped) return f.error = "column '" + e.name + "' is a nested field (a group of " + std::to_string(e.children) + ")", f;
            const Element& el = elements[k + 2];
            Leaf leaf;
            leaf.name = e.name, leaf.physical = el.type, leaf.required = e.repetition == 0, leaf.list = true;
            leaf.def_list = e.repetition == 1, leaf.def_slot = leaf.def_list + 1, leaf.max_def = leaf.def_slot + (el.repetition == 1);
            if (!list_element_read(el.type)) leaf.cause = std::string("a list of ") + physical_name(el.type) + " is not read";
            f.leaves.push_back(std::move(leaf));
            k += 3;
            continue;
        }
        if (e.repetition == 2) return f.error = "column '" + e.name + "' is a repeated field (repetition levels are not read)", f;
        Leaf leaf;
        leaf.name = e.name, leaf.physical = e.type, leaf.required = e.repetition == 0;
        if (!native_type(e.type)) leaf.cause = std::string(physical_name(e.type)) + " is not read";
        f.leaves.push_back(std::move(leaf));
        ++k;
    }
    if ((uint64_t)elements[0].children != children)
        return f.error = "the schema's root names " + std::to_string(elements[0].children) + " children, the schema has " + std::to_string(children), f;
    if ((uint64_t)num_rows > kMaxRows) return f.error = "more than 2^40 rows", f;
    f.nrows = (uint64_t)num_rows;
    const uint64_t ncols = f.leaves.size();
    uint64_t sum = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const std::string where = "row group " + std::to_string(g);
        if (groups[g].size() != ncols) return f.error = where + " has " + std::to_string(groups[g].size()) + " column chunks, the schema " + std::to_string(ncols) + " columns", f;
        if (group_rows[g] < 0 || (uint64_t)group_rows[g] > kMaxRows) return f.error = where + " has no valid num_rows", f;
        for (uint64_t c = 0; c < ncols; ++c) {
            const ChunkMeta& m = groups[g][c];
            const std::string col = where + ", column '" + f.leaves[c].name + "'";
            if (!m.has_meta || m.encrypted) return f.error = col + ": its chunk has no plain metadata in the footer", f;
            if (m.codec != kCodecNone && !(inflate && m.codec == kCodecSnappy) && !(zstd && m.codec == kCodecZstd))
                return f.error = col + ": compression codec " + std::to_string(m.codec) +
                                 (zstd ? (inflate ? " (UNCOMPRESSED, 0, SNAPPY, 1, and ZSTD, 6, are read on the device)"
                                                  : " (UNCOMPRESSED, 0, and ZSTD, 6, are read on the device; OXH_PARQUET_INFLATE adds SNAPPY, 1)")
                                  : inflate ? " (UNCOMPRESSED, 0, and SNAPPY, 1, are read on the device)"
                                          : " (only UNCOMPRESSED, 0, is read on the device; OXH_PARQUET_INFLATE adds SNAPPY, 1)"), f;
            const int64_t first = m.dict_at > 0 && m.dict_at < m.data_at ? m.dict_at : m.data_at;
            if (first < 4 || m.compressed < 0 || (uint64_t)first > meta_at || (uint64_t)m.compressed > meta_at - (uint64_t)first)
                return f.error = col + ": its chunk (" + std::to_string(m.compressed) + " bytes at " + std::to_string(first) + ") is not inside the file's " +
                                 std::to_string(nbytes) + " bytes in front of the footer", f;
            // a list's chunk counts level entries: every row has one at least
            if (f.leaves[c].list ? m.num_values < group_rows[g] : m.num_values != group_rows[g])
                return f.error = col + ": num_values " + std::to_string(m.num_values) + (f.leaves[c].list ? " is less than the group's " : " is not the group's ") +
                                 std::to_string(group_rows[g]) + " rows", f;
            f.chunks.push_back(Chunk{(uint64_t)first, (uint64_t)m.compressed, (uint64_t)m.num_values, (uint32_t)m.codec});
        }
        f.group_rows.push_back((uint64_t)group_rows[g]);
        sum += (uint64_t)group_rows[g];
    }
    if (sum != f.nrows) return f.error = "the row groups hold " + std::to_string(sum) + " rows, num_rows is " + std::to_string(f.nrows), f;
    return f;
}

// ---------------------------------------------------------------- the page table
// What the walk kernel reads per chunk and leaves per page.
struct ChunkDesc {
    uint64_t at, bytes, num_values;
    uint32_t optional, page0;  // page0: where its records start in the table (the fill pass)
    uint32_t codec, pad;
};

struct PageRec {
    uint64_t body;  // where the page's body starts in the file; once inflated (kPageInImage), in the handle's image
    uint32_t body_size, kind, num_values, encoding;  // body_size: of the body the column kernels read (the inflated one)
    uint32_t def_at, def_bytes, values_at;  // in the body: the definition levels' runs, then the values
    uint32_t flags;                         // bit 0: repetition levels, bit 1: a V1 level encoding that is not RLE, kPage*
    uint32_t file_size, stored;             // the body's bytes in the file; of those, a V2 page's levels, stored as they are
};
constexpr uint32_t kPageInImage = 4;      // a compressed page: its body is inflated into the image
constexpr uint32_t kPageLevelsLater = 8;  // a compressed V1 page of an OPTIONAL column: its levels' length is in the inflated body
constexpr uint32_t kPageZstd = 16;        // a compressed page of a ZSTD chunk: a Zstandard frame, not a Snappy block

// A compressed V1 page's levels, once the first 4 bytes of its inflated body (`def_bytes`) are known: what the walk
// leaves of a page that is not compressed.
OXH_PQR_BOTH void finish_v1_levels(PageRec& r, uint32_t def_bytes) {
    r.def_at = 4, r.def_bytes = def_bytes;
    r.values_at = r.body_size >= 4 && def_bytes <= r.body_size - 4 ? 4 + def_bytes : ~0u;  // ~0u: column_pages refuses it
    r.flags &= ~kPageLevelsLater;
}

// The image of the compressed pages: each inflated body in table order on a 16-byte grid. places[k]: where page k's
// body starts in it (compressed pages only). A page whose claimed size no stream of its codec reaches stops the plan:
// `implausible` is that page, else ~0.
struct ImagePlan {
    std::vector<uint64_t> places;
    uint64_t bytes = 0, pages = 0, implausible = ~0ull;
};
inline ImagePlan plan_image(const std::vector<PageRec>& recs) {
    ImagePlan plan;
    plan.places.assign(recs.size(), 0);
    for (size_t k = 0; k < recs.size(); ++k) {
        const PageRec& r = recs[k];
        if (!(r.flags & kPageInImage)) continue;
        if (r.stored > r.file_size || r.stored > r.body_size ||
            !(r.flags & kPageZstd ? zstd_size_plausible : inflated_size_plausible)(r.file_size - r.stored, r.body_size - r.stored))
            return plan.implausible = k, plan;
        plan.places[k] = plan.bytes, plan.bytes += ((uint64_t)r.body_size + 15) & ~15ull, ++plan.pages;
    }
    return plan;
}

// What the column kernels read per data page and per dictionary page of one column.
struct DataPage {
    uint64_t row0, word0;  // its first row; its first word of the column's page-local validity words
    uint64_t body;
    uint32_t num_values, body_size, def_at, def_bytes, values_at, encoding;
    uint32_t dict;         // its chunk's dictionary page in the column's list, ~0u: none
    uint32_t in_image;     // its body is at `body` of the handle's image, not of the file
};
struct DictPage {
    uint64_t body, entry0;  // entry0: its first entry in the column's dictionary tables
    uint32_t body_size, num_values;
    uint32_t in_image, pad;
};

// A data page of a list column (parquet_lists.hip). Its num_values are level entries, not rows: `word0` is its first
// word of the column's level words, 64 entries a word, and word0 * 64 its first cell of the column's index array.
// V2: both streams' places are the header's. V1 (def_at == ~0u): the repetition stream's length led the body; the
// definition stream's own 4-byte length is at `values_at`, and the level kernel reads it, bounded by body_size.
struct ListPage {
    uint64_t body, word0;
    uint32_t num_values, body_size;
    uint32_t rep_at, rep_bytes, def_at, def_bytes, values_at;
    uint32_t encoding, dict, in_image;
    uint32_t first;  // its chunk's first data page: its first entry must start a row
    uint32_t group;  // its row group
};

struct ColumnPages {
    std::vector<DataPage> data;
    std::vector<ListPage> lists;  // a list column's data pages; `data` is then empty
    std::vector<DictPage> dicts;
    uint64_t words = 0, entries = 0;
    bool indices = false;  // a page whose values are indices or RLE booleans
    std::string cause;     // not empty: why this reader cannot read the column's pages
};

// The pages of column c (the records of its chunks, group after group) checked and listed. A refusal is the
// column's own: it stops the column, not the file.
inline ColumnPages column_pages(const Footer& f, uint64_t c, const std::vector<ChunkDesc>& chunks, const std::vector<uint32_t>& counts,
                                const std::vector<PageRec>& recs) {
    ColumnPages out;
    const uint64_t ncols = f.leaves.size();
    const int32_t physical = f.leaves[c].physical;
    uint64_t row0 = 0;
    for (size_t g = 0; g < f.group_rows.size(); ++g) {
        const size_t ch = g * ncols + c;
        uint32_t dict = ~0u;
        for (uint32_t k = 0; k < counts[ch]; ++k) {
            const PageRec& r = recs[chunks[ch].page0 + k];
            const std::string where = "row group " + std::to_string(g) + ", page " + std::to_string(k);
            if (r.values_at > r.body_size || r.def_at > r.values_at || r.def_bytes > r.values_at - r.def_at)
                return out.cause = where + ": its levels do not fit its " + std::to_string(r.body_size) + " bytes", out;
            if (r.kind == (uint32_t)kPageDict) {
                if (k != 0) return out.cause = where + ": a dictionary page that is not its chunk's first page", out;
                if (r.encoding != (uint32_t)kEncPlain && r.encoding != (uint32_t)kEncPlainDict)
                    return out.cause = where + ": dictionary encoding " + std::to_string(r.encoding) + " is not read", out;
                if (physical == kBoolean) return out.cause = where + ": a dictionary of booleans", out;
                dict = (uint32_t)out.dicts.size();
                out.dicts.push_back(DictPage{r.body, out.entries, r.body_size, r.num_values, r.flags & kPageInImage ? 1u : 0u, 0});
                out.entries += r.num_values;
                continue;
            }
            if (r.kind != (uint32_t)kPageData && r.kind != (uint32_t)kPageDataV2) return out.cause = where + ": page type " + std::to_string(r.kind) + " is not read", out;
            if (r.flags & 1) return out.cause = where + ": repetition levels are not read", out;
            if (r.flags & 2) return out.cause = where + ": definition levels that are not RLE", out;
            const bool indexed = r.encoding == (uint32_t)kEncPlainDict || r.encoding == (uint32_t)kEncRleDict;
            const bool rle_bool = r.encoding == (uint32_t)kEncRle && physical == kBoolean;
            if (r.encoding != (uint32_t)kEncPlain && !indexed && !rle_bool)
                return out.cause = where + ": value encoding " + std::to_string(r.encoding) + " is not read (PLAIN, the dictionary encodings, RLE booleans)", out;
            if (indexed && dict == ~0u) return out.cause = where + ": dictionary-coded values without a dictionary page", out;
            out.indices |= indexed || rle_bool;
            out.data.push_back(DataPage{row0, out.words, r.body, r.num_values, r.body_size, r.def_at, r.def_bytes, r.values_at, r.encoding,
                                        indexed ? dict : ~0u, r.flags & kPageInImage ? 1u : 0u});
            row0 += r.num_values, out.words += (r.num_values + 63) / 64;
        }
    }
    if (row0 != f.nrows) return out.cause = "its pages hold " + std::to_string(row0) + " values, the file " + std::to_string(f.nrows) + " rows", out;
    return out;
}

// The same for a list column: its pages carry repetition levels, and nothing says where a row starts but they. A
// page may begin in the middle of a row, except its chunk's first.
inline ColumnPages list_pages(const Footer& f, uint64_t c, const std::vector<ChunkDesc>& chunks, const std::vector<uint32_t>& counts,
                              const std::vector<PageRec>& recs) {
    ColumnPages out;
    const uint64_t ncols = f.leaves.size();
    for (size_t g = 0; g < f.group_rows.size(); ++g) {
        const size_t ch = g * ncols + c;
        uint32_t dict = ~0u;
        bool first = true;
        for (uint32_t k = 0; k < counts[ch]; ++k) {
            const PageRec& r = recs[chunks[ch].page0 + k];
            const std::string where = "row group " + std::to_string(g) + ", page " + std::to_string(k);
            if (r.values_at > r.body_size || r.def_at > r.values_at || r.def_bytes > r.values_at - r.def_at)
                return out.cause = where + ": its levels do not fit its " + std::to_string(r.body_size) + " bytes", out;
            if (r.kind == (uint32_t)kPageDict) {
                if (k != 0) return out.cause = where + ": a dictionary page that is not its chunk's first page", out;
                if (r.encoding != (uint32_t)kEncPlain && r.encoding != (uint32_t)kEncPlainDict)
                    return out.cause = where + ": dictionary encoding " + std::to_string(r.encoding) + " is not read", out;
                dict = (uint32_t)out.dicts.size();
                out.dicts.push_back(DictPage{r.body, out.entries, r.body_size, r.num_values, r.flags & kPageInImage ? 1u : 0u, 0});
                out.entries += r.num_values;
                continue;
            }
            if (r.kind != (uint32_t)kPageData && r.kind != (uint32_t)kPageDataV2) return out.cause = where + ": page type " + std::to_string(r.kind) + " is not read", out;
            if (r.flags & 2) return out.cause = where + ": levels that are not RLE", out;
            const bool indexed = r.encoding == (uint32_t)kEncPlainDict || r.encoding == (uint32_t)kEncRleDict;
            if (r.encoding != (uint32_t)kEncPlain && !indexed)
                return out.cause = where + ": value encoding " + std::to_string(r.encoding) + " is not read (PLAIN, the dictionary encodings)", out;
            if (indexed && dict == ~0u) return out.cause = where + ": dictionary-coded values without a dictionary page", out;
            out.indices |= indexed;
            const bool v1 = r.kind == (uint32_t)kPageData;  // the walk left the repetition stream where a flat page has its definition levels
            out.lists.push_back(ListPage{r.body, out.words, r.num_values, r.body_size, v1 ? 4u : 0u, v1 ? r.def_bytes : r.def_at, v1 ? ~0u : r.def_at,
                                         v1 ? 0u : r.def_bytes, r.values_at, r.encoding, indexed ? dict : ~0u, r.flags & kPageInImage ? 1u : 0u,
                                         first ? 1u : 0u, (uint32_t)g});
            out.words += ((uint64_t)r.num_values + 63) / 64, first = false;
        }
    }
    return out;
}

// oxh_parquet_lists_*'s arguments (after the handle itself was checked): "" when they are well formed, else what is
// wrong with them, in the header's order. All four output tables NULL: the call only measures.
struct ListsArgs {
    uint64_t nrows, ncols;  // of the handle
    uint32_t nsel;
    const uint32_t* col_idx;
    const uint32_t* types;
    const uint64_t* value_capacity;
    void* const* values;
    void* const* offsets;
    uint8_t* const* validity;
    uint8_t* const* child_validity;
    uint64_t* value_bytes;
    uint64_t* stats4;
};
inline uint32_t list_cell_bytes(uint32_t type) { return csv::is_narrow(element_word(type)) ? 4 : 8; }
inline std::string lists_error(const ListsArgs& a) {
    if (a.nsel && (!a.col_idx || !a.types)) return "col_idx or types is NULL";
    for (uint32_t k = 0; k < a.nsel; ++k)
        if (a.col_idx[k] >= a.ncols) return "selection " + std::to_string(k) + " names column " + std::to_string(a.col_idx[k]) + " of " + std::to_string(a.ncols);
    for (uint32_t k = 0; k < a.nsel; ++k) {
        const uint32_t e = element_word(a.types[k]);
        if (!is_list_word(a.types[k]) || (e != OXH_CSV_INT64 && e != OXH_CSV_FLOAT64 && e != OXH_CSV_INT32 && e != OXH_CSV_FLOAT32))
            return "selection " + std::to_string(k) + " has type " + std::to_string(a.types[k]) + ", which is not OXH_PARQUET_LIST on a fixed-width element's word";
    }
    if (a.nsel && (!a.value_bytes || !a.stats4)) return "value_bytes or stats4 is NULL";
    const bool measure = !a.values && !a.offsets && !a.validity && !a.child_validity;
    if (measure || !a.nsel) return "";
    if (!a.values || !a.offsets || !a.validity || !a.child_validity) return "only some of values, offsets, validity and child_validity are NULL";
    if (!a.value_capacity) return "value_capacity is NULL with outputs";
    if (!a.nrows) return "";
    for (uint32_t k = 0; k < a.nsel; ++k) {
        const std::string col = "selection " + std::to_string(k);
        if (!a.validity[k]) return col + " has no validity buffer";
        if (!a.offsets[k]) return col + " has no offsets";
        if ((uintptr_t)a.offsets[k] & (a.types[k] & OXH_PARQUET_LIST64 ? 7 : 3)) return col + ": offsets is not aligned to its entries";
        if (a.value_capacity[k] && (!a.values[k] || !a.child_validity[k])) return col + " has a capacity but no values or no child_validity";
        if ((uintptr_t)a.values[k] & (list_cell_bytes(a.types[k]) - 1)) return col + ": values is not aligned to its cells";
    }
    return "";
}

// "" when the pages' row starts (one count per page of cp.lists) are every row group's rows.
inline std::string list_rows_error(const Footer& f, const ColumnPages& cp, const uint32_t* starts) {
    std::vector<uint64_t> rows(f.group_rows.size(), 0);
    for (size_t p = 0; p < cp.lists.size(); ++p) rows[cp.lists[p].group] += starts[p];
    for (size_t g = 0; g < rows.size(); ++g)
        if (rows[g] != f.group_rows[g])
            return "row group " + std::to_string(g) + ": its pages start " + std::to_string(rows[g]) + " rows, the group has " + std::to_string(f.group_rows[g]);
    return "";
}

}  // namespace oxh::pqr
