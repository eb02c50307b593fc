// tests/native/parquet_dict_host_test.cpp -- what parquet_host.hpp adds for OXH_PARQUET_DICTIONARY, on the CPU: the
// fallback decision at each of its three limits, the index width, the index stream's bytes, and the plan over
// hand-made tile and chunk tables -- the dictionary page in front of its chunk, the data pages cut by the index
// stream, the dictionary page's header bytes, the dense spans, the footer's offsets as the reader's planner sees them -- alone and
// with stored (SNAPPY) sizes, under snappy_capacity(). Also what a sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"
#include "../../oxen_amd/csrc/parquet_read_host.hpp"

namespace pq = oxh::parquet;
namespace pr = oxh::pqr;

static int64_t zigzag_at(const std::vector<uint8_t>& b, size_t& p) {
    uint64_t v = 0;
    for (int shift = 0;; shift += 7) {
        const uint8_t byte = b.at(p++);
        v |= (uint64_t)(byte & 0x7F) << shift;
        if (!(byte & 0x80)) break;
    }
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
}

static void limits() {
    const pq::ChunkDict ok{pq::kDictMaxEntries, 8 * pq::kDictMaxEntries, 0};
    assert(pq::dict_chunk(OXH_CSV_INT64, ok) && pq::dict_chunk(OXH_CSV_STRING, ok) && !pq::dict_chunk(OXH_CSV_BOOL, ok));
    assert(!pq::dict_chunk(OXH_CSV_INT64, pq::ChunkDict{pq::kDictMaxEntries + 1, 8, 0}));   // too many values
    assert(pq::dict_chunk(OXH_CSV_STRING, pq::ChunkDict{5, pq::kDictMaxPage, 0}));
    assert(!pq::dict_chunk(OXH_CSV_STRING, pq::ChunkDict{5, pq::kDictMaxPage + 1, 0}));    // the page's body above 1 MiB
    assert(!pq::dict_chunk(OXH_CSV_STRING, pq::ChunkDict{5, 40, 1}));                      // a cell above kDictMaxCell (or the count)
    assert(!pq::dict_chunk(OXH_CSV_FLOAT64, pq::ChunkDict{0, 0, 0}));                      // every cell null
    const uint64_t n[] = {1, 2, 3, 4, 5, 256, 257, 65535, 65536};
    const uint32_t w[] = {1, 1, 2, 2, 3, 8, 9, 16, 16};
    for (int k = 0; k < 9; ++k) assert(pq::dict_width(n[k]) == w[k]);
    assert(pq::index_stream_len(0, 7) == 1 && pq::index_stream_len(1, 7) == 1 + 1 + 7 && pq::index_stream_len(8, 9) == 1 + 1 + 9);
    assert(pq::index_stream_len(9, 1) == 1 + 1 + 2 && pq::index_stream_len(512, 3) == 1 + 2 + 64 * 3);   // 64 groups: a 2-byte varint
}

// INT64 with nulls (`values` distinct values a chunk) beside a string column that falls back and a boolean.
static void check(uint64_t nrows, uint64_t rows_per_group, uint64_t page_bytes, uint64_t values, bool snappy) {
    const uint32_t types[3] = {OXH_CSV_INT64, OXH_CSV_STRING, OXH_CSV_BOOL};
    const uint8_t names[] = "isb";
    const uint64_t name_offsets[4] = {0, 1, 2, 3};
    const uint64_t group = pq::group_rows_of(rows_per_group), ntiles = (nrows + pq::kTileRows - 1) / pq::kTileRows, ngroups = (nrows + group - 1) / group;
    std::vector<pq::Tile> tiles(ntiles * 3 + 1);
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t rows = std::min(nrows - t * pq::kTileRows, pq::kTileRows);
        tiles[3 * t] = pq::Tile{8 * (rows - rows / 3), 1, 9, (uint32_t)(rows - rows / 3), 1};
        tiles[3 * t + 1] = pq::Tile{rows * 9, 0, 0, (uint32_t)rows, 0};
        tiles[3 * t + 2] = pq::Tile{rows, 0, 0, (uint32_t)rows, 0};
    }
    std::vector<pq::ChunkDict> dicts(ngroups * 3 + 1);
    for (uint64_t g = 0; g < ngroups; ++g) dicts[3 * g] = pq::ChunkDict{values, 8 * values, 0}, dicts[3 * g + 1] = pq::ChunkDict{7, 70, 1}, dicts[3 * g + 2] = pq::ChunkDict{~0ull, ~0ull, ~0ull};
    pq::Plan p = pq::make_plan(nrows, 3, types, names, name_offsets, rows_per_group, page_bytes, tiles.data(), nullptr, dicts.data());
    assert(p.error.empty() && p.header_len.size() == p.pages.size() && p.row_groups == ngroups);
    const uint64_t capacity = pq::snappy_capacity(p, 3);
    std::vector<uint64_t> kept(p.pages.size() + 1);
    if (snappy) {   // every body at Snappy's bound: the largest file the capacity has to hold
        for (size_t k = 0; k < p.pages.size(); ++k) {
            const uint64_t body = p.pages[k].head_len - p.header_len[k] + p.pages[k].level_bytes + p.pages[k].values_bytes;
            kept[k] = 32 + body + body / 6;
        }
        const size_t np = p.pages.size();
        p = pq::make_plan(nrows, 3, types, names, name_offsets, rows_per_group, page_bytes, tiles.data(), kept.data(), dicts.data());
        assert(p.error.empty() && p.pages.size() == np && p.out_bytes <= capacity);
    }
    const uint32_t w = pq::dict_width(values);
    uint64_t at = 4, dense = 0, ndict = 0;
    for (size_t k = 0; k < p.pages.size(); ++k) {
        const pq::Page& pg = p.pages[k];
        assert(pg.file_at == at);
        size_t q = pg.head_src;
        if (pg.col != 0) {   // the fallback chunks and the booleans: what the plan without dictionaries has
            assert(!pg.dict_width && pg.rows && p.blob.at(q++) == 0x15 && zigzag_at(p.blob, q) == 0);
        } else if (!pg.rows) {   // the dictionary page: DICTIONARY_PAGE, its sizes, DictionaryPageHeader{num_values, PLAIN}
            assert(pg.dict_page == k && pg.dict_width == w && pg.nvalid == values && pg.head_len == p.header_len[k] && pg.level_bytes == 0);
            assert(p.blob.at(q++) == 0x15 && zigzag_at(p.blob, q) == 2);
            assert(p.blob.at(q++) == 0x15 && zigzag_at(p.blob, q) == (int64_t)(8 * values));
            assert(p.blob.at(q++) == 0x15 && zigzag_at(p.blob, q) == (int64_t)(snappy ? kept[k] : 8 * values));
            assert(p.blob.at(q++) == 0x4C && p.blob.at(q++) == 0x15 && zigzag_at(p.blob, q) == (int64_t)values);
            assert(p.blob.at(q++) == 0x15 && zigzag_at(p.blob, q) == 0 && p.blob.at(q++) == 0 && p.blob.at(q++) == 0 && q == pg.head_src + pg.head_len);
            assert(pg.values_bytes == (snappy ? kept[k] : 8 * values));
            ++ndict;
        } else {   // an RLE_DICTIONARY data page: cut by the index stream, its span of the dense array
            assert(pg.dict_width == w && pg.dict_page < k && !p.pages[pg.dict_page].rows && p.pages[pg.dict_page].col == 0);
            assert(pg.dense_at == dense && dense % pq::kDenseBlock == 0);
            dense += (pg.nvalid + pq::kDenseBlock - 1) / pq::kDenseBlock * pq::kDenseBlock;
            if (!snappy) assert(pg.values_bytes == pq::index_stream_len(pg.nvalid, w));
            if (pg.rows > pq::kTileRows)   // a page stops at the first tile with which it reaches the budget
                assert(4 + pq::level_run_len(pg.rows - pq::kTileRows, true) + pq::index_stream_len(pg.nvalid - (pq::kTileRows - pq::kTileRows / 3), w) < pq::page_bytes_of(page_bytes));
        }
        at += snappy ? p.header_len[k] + pg.values_bytes : pg.head_len + pg.level_bytes + pg.values_bytes;
    }
    assert(ndict == ngroups && dense == p.dense_indices && p.out_bytes == at + p.footer.size());
    // the footer as the reader's planner sees it: a dictionary chunk starts at its dictionary page
    const pr::Footer f = pr::read_footer(p.footer.data(), p.footer.size() - 8, at, p.out_bytes, snappy);
    assert(f.error.empty() && f.nrows == nrows && f.chunks.size() == 3 * ngroups);
    uint64_t next = 4;
    for (const pr::Chunk& c : f.chunks) {
        assert(c.at == next);
        next += c.bytes;
    }
    assert(next == at);
}

int main() {
    limits();
    for (int snappy = 0; snappy < 2; ++snappy) {
        check(1, 0, 0, 1, snappy);
        check(2049, 1024, 4096, 3, snappy);        // one-tile groups: a dictionary per chunk
        check(20000, 8192, 4096, 257, snappy);     // width 9: 3 tiles a page, pages cut mid-chunk
        check(300000, 0, 0, 65536, snappy);        // the largest dictionary, one page of indices
        check(300000, 131072, 65536, 100, snappy);
    }
    std::puts("ok");
    return 0;
}
