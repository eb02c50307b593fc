// tests/native/parquet_snappy_host_test.cpp -- what parquet_host.hpp adds for OXH_PARQUET_SNAPPY, on the CPU: the plan
// made again with the pages' stored sizes -- compressed_page_size beside uncompressed_page_size in every PageHeader,
// the pages' places, codec SNAPPY, the chunks' and row groups' stored and uncompressed totals, the file's size -- for
// stored sizes below, at and above the bodies and on both sides of every varint's byte boundary, and that
// snappy_capacity() of the uncompressed plan holds every such file. Also what a sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"
#include "../../oxen_amd/csrc/parquet_read_host.hpp"

namespace pq = oxh::parquet;
namespace pr = oxh::pqr;

// The zigzag varint at p: its value; p moves behind it.
static int64_t zigzag_at(const std::vector<uint8_t>& b, size_t& p) {
    uint64_t v = 0;
    for (int shift = 0;; shift += 7) {
        const uint8_t byte = b.at(p++);
        v |= (uint64_t)(byte & 0x7F) << shift;
        if (!(byte & 0x80)) break;
    }
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
}

static uint64_t body_of(const pq::Plan& plain, size_t k) {
    const pq::Page& pg = plain.pages[k];
    return pg.head_len - plain.header_len[k] + pg.level_bytes + pg.values_bytes;
}

// One frame (INT64 with nulls, STRING) of `nrows` rows whose tiles hold `cell` string bytes a row.
static void check(uint64_t nrows, uint64_t rows_per_group, uint64_t page_bytes, uint64_t cell) {
    const uint32_t types[2] = {OXH_CSV_INT64, OXH_CSV_STRING};
    const uint8_t names[] = "is";
    const uint64_t name_offsets[3] = {0, 1, 2};
    const uint64_t ntiles = (nrows + pq::kTileRows - 1) / pq::kTileRows;
    std::vector<pq::Tile> tiles(ntiles * 2 + 1);
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t rows = std::min(nrows - t * pq::kTileRows, pq::kTileRows);
        tiles[2 * t] = pq::Tile{8 * (rows - rows / 3), 1, 9, (uint32_t)(rows - rows / 3), 1};
        tiles[2 * t + 1] = pq::Tile{rows * (4 + cell), 0, 0, (uint32_t)rows, 0};
    }
    const pq::Plan plain = pq::make_plan(nrows, 2, types, names, name_offsets, rows_per_group, page_bytes, tiles.data());
    assert(plain.error.empty() && plain.header_len.size() == plain.pages.size() && plain.stored_bytes == plain.plain_bytes);
    const uint64_t capacity = pq::snappy_capacity(plain, 2);
    const size_t np = plain.pages.size();
    // stored sizes: tiny, the body, Snappy's bound of it, and the two sides of the varints' byte boundaries
    const uint64_t edges[] = {1, 63, 64, 8191, 8192, 1048575, 1048576};
    for (int mode = 0; mode < 3 + (int)(sizeof(edges) / sizeof(edges[0])); ++mode) {
        std::vector<uint64_t> kept(np + 1);
        for (size_t k = 0; k < np; ++k) {
            const uint64_t body = body_of(plain, k), bound = 32 + body + body / 6;
            kept[k] = mode == 0 ? 1 + k % 3 : mode == 1 ? body : mode == 2 ? bound : std::min(edges[mode - 3] + k % 2, bound);
        }
        const pq::Plan sp = pq::make_plan(nrows, 2, types, names, name_offsets, rows_per_group, page_bytes, tiles.data(), kept.data());
        assert(sp.error.empty() && sp.pages.size() == np && sp.header_len.size() == np && sp.row_groups == plain.row_groups);
        uint64_t at = 4, stored = 0, unpacked = 0;
        for (size_t k = 0; k < np; ++k) {
            const pq::Page &pg = sp.pages[k], &was = plain.pages[k];
            assert(pg.file_at == at && pg.values_bytes == kept[k] && pg.rows == was.rows && pg.col == was.col && pg.tile0 == was.tile0);
            // the PageHeader: type, uncompressed_page_size, compressed_page_size
            size_t p = pg.head_src;
            assert(sp.blob.at(p++) == 0x15 && zigzag_at(sp.blob, p) == 0);
            assert(sp.blob.at(p++) == 0x15 && zigzag_at(sp.blob, p) == (int64_t)body_of(plain, k));
            assert(sp.blob.at(p++) == 0x15 && zigzag_at(sp.blob, p) == (int64_t)kept[k]);
            assert(sp.header_len[k] <= plain.header_len[k] + 4 && sp.header_len[k] + 4 >= plain.header_len[k]);
            at += sp.header_len[k] + kept[k], stored += sp.header_len[k] + kept[k], unpacked += sp.header_len[k] + body_of(plain, k);
        }
        assert(sp.stored_bytes == stored && sp.plain_bytes == unpacked && sp.out_bytes == at + sp.footer.size());
        assert(sp.out_bytes <= capacity);  // every arm keeps its bodies at or below Snappy's bound
        // the footer as the reader sees it: every chunk SNAPPY, where its first page is, with the bytes of its pages
        const uint64_t meta = sp.footer.size() - 8;
        const pr::Footer f = pr::read_footer(sp.footer.data(), meta, at, sp.out_bytes, true);
        assert(f.error.empty() && f.nrows == nrows && f.chunks.size() == 2 * sp.row_groups);
        uint64_t sum = 0, next = 4;
        for (const pr::Chunk& c : f.chunks) {
            assert((np == 0 || c.codec == pr::kCodecSnappy) && c.at == next);
            sum += c.bytes, next += c.bytes;
        }
        assert(sum == stored);
        assert(!pr::read_footer(sp.footer.data(), meta, at, sp.out_bytes, false).error.empty() || np == 0);  // refused without the flag
    }
}

int main() {
    assert(pq::write_error(pq::Args{}, true) != "unknown flags");
    check(0, 0, 0, 3);
    check(1, 0, 0, 0);
    check(5000, 2048, 4096, 7);          // one-tile pages, three row groups
    check(300000, 131072, 0, 30);        // pages at the default budget: bodies above 1 MiB
    check(2049, 1024, 1 << 20, 70000);   // huge cells: a page per tile, 70 MB each
    std::puts("ok");
    return 0;
}
