// tests/native/parquet_write_lists_host_test.cpp -- parquet_host.hpp's list columns on the CPU: the level heads, both
// forms of both streams, at entry counts 1, 7, 8 and 9; the planner over hand-made list tiles (page cuts by entries,
// the pages' entry and value bases, the body's layout, refusals); the list argument errors' spans. Also what a
// sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"

namespace pq = oxh::parquet;

static pq::Tile tile(uint32_t lists, uint64_t entries, uint64_t values, uint32_t width) {
    pq::Tile t{};
    t.valid = lists, t.min = entries, t.value_bytes = values * width;
    return t;
}

int main() {
    // level heads: {u32 length, run header, RLE's value byte}; n <= 63 keeps every varint one byte
    for (uint64_t n : {1, 7, 8, 9}) {
        const uint8_t groups = (uint8_t)((n + 7) / 8);
        for (uint32_t width : {1u, 2u}) {
            pq::Thrift rle, packed;
            pq::put_level_head(rle, n, width, true, width == 1 ? 0 : 3);
            pq::put_level_head(packed, n, width, false, 0);
            const std::vector<uint8_t> want_rle{2, 0, 0, 0, (uint8_t)(n << 1), (uint8_t)(width == 1 ? 0 : 3)};
            const std::vector<uint8_t> want_packed{(uint8_t)(1 + groups * width), 0, 0, 0, (uint8_t)((groups << 1) | 1)};
            assert(rle.out == want_rle && packed.out == want_packed);
            assert(pq::level_packed_bytes(n, width, true) == 0 && pq::level_packed_bytes(n, width, false) == (uint64_t)groups * width);
            assert(pq::level_stream_len(n, width, true) == 2 && pq::level_stream_len(n, width, false) == 1ull + groups * width);
        }
        assert(pq::list_body_len(n, n, n, 4) == 8 + 2 + 2 + 4 * n);                        // a row an entry, all values: both RLE
        assert(pq::list_body_len(1, n + 1, n, 8) == 8 + 2 * (1 + (n + 8) / 8) + (n + 8) / 8 + 8 * n);  // both bit-packed
    }
    // the planner: 2 100 rows of list<int32> beside an int64 column, row groups of 2 048, pages of 4 096 bytes
    const uint32_t types[2] = {OXH_PARQUET_LIST | OXH_CSV_INT32, OXH_CSV_INT64};
    const uint8_t names[] = "vid";
    const uint64_t name_offsets[3] = {0, 1, 3};
    std::vector<pq::Tile> tiles;
    tiles.push_back(tile(1024, 1024, 1024, 4)), tiles.push_back(tile(1024, 0, 0, 1)), tiles.back().value_bytes = 8192;   // a value a row: both streams RLE
    tiles.push_back(tile(1000, 3000, 2500, 4)), tiles.push_back(tiles[1]);
    tiles.push_back(tile(52, 52, 0, 4)), tiles.push_back(tile(52, 0, 0, 1)), tiles.back().value_bytes = 416;             // empty lists only
    const pq::Plan p = pq::make_plan(2100, 2, types, names, name_offsets, 2048, 4096, tiles.data());
    assert(p.error.empty() && p.row_groups == 2 && p.pages.size() == 6 && p.null_cells == 24);
    uint64_t at = 4;
    for (const pq::Page& g : p.pages) {
        assert(g.file_at == at && g.head_len + g.def_head_len < 64 && g.head_src + g.head_len + g.def_head_len <= p.blob.size());
        at += g.head_len + g.level_bytes + g.values_bytes;
    }
    assert(at + p.footer.size() == p.out_bytes);
    const pq::Page &a = p.pages[0], &b = p.pages[1], &c = p.pages[4];
    assert(a.col == 0 && a.rows == 1024 && a.entries == 1024 && a.nvalid == 1024 && a.entry0 == 0 && a.def_head_len == 7 && a.level_bytes == 7 && a.values_bytes == 4096);
    assert(b.col == 0 && b.rows == 1024 && b.entries == 3000 && b.nvalid == 2500 && b.entry0 == 1024 && b.value0 == 1024 && b.tile0 == 1);
    assert(b.def_head_len == 6 && b.level_bytes == 375 + 6 + 750 && b.values_bytes == 10000);
    assert(c.col == 0 && c.entries == 52 && c.nvalid == 0 && c.entry0 == 4024 && c.value0 == 3524 && c.def_head_len == 5 && c.level_bytes == 5 + 14 && c.values_bytes == 0);
    // the bodies' bytes behind the PageHeader: page 1 is {rep length, bit-packed header}{375 B}{def length, header}{750 B}
    const uint8_t* h = p.blob.data() + b.head_src + p.header_len[1];
    assert(b.head_len - p.header_len[1] == 6 && h[0] == (377 & 0xFF) && h[1] == 377 >> 8 && h[4] == ((((375 << 1) | 1) & 0x7F) | 0x80) && h[6] == (752 & 0xFF));
    // refusals: a tile with fewer entries than rows, more values than entries, a page of 2^31 entries
    const pq::Tile few = tile(1024, 1000, 0, 4), many = tile(1024, 1024, 1025, 4), huge = tile(1024, 1ull << 31, 0, 4);
    for (const pq::Tile* t : {&few, &many, &huge}) assert(!pq::make_plan(1024, 1, types, names, name_offsets, 0, 0, t).error.empty());
    // the argument checks: kinds, the element's word, the offsets' alignment, the span of the lists that are not null
    assert(pq::kind_of(types[0]) == OXH_COL_FIXED4 && pq::kind_of(OXH_PARQUET_LIST | OXH_PARQUET_LIST64 | OXH_CSV_FLOAT64) == OXH_COL_FIXED8);
    const int32_t offsets[5] = {7, 9, 2, 12, 12};  // row 1 is null and runs backwards: never read through
    const uint8_t valid = 0x0D;
    const uint32_t kinds[1] = {OXH_COL_FIXED4};
    const void* tables[2] = {nullptr, offsets};
    const uint8_t* bitmaps[1] = {&valid};
    const uint64_t bits[2] = {0, 0};
    uint64_t size = 0, stats4[4];
    pq::Args args{4, 1, types, kinds, tables, tables + 1, bitmaps, bits, names, name_offsets, 0, 0, 0, nullptr, 0, &size, stats4};
    const pq::ListSpan span = pq::list_span(args, 0);
    assert(span.bad_row == 4 && span.lo == 2 && span.hi == 12);
    assert(pq::write_error(args, true).find("has elements but no values") != std::string::npos && pq::write_error(args, false).empty());
    const void* odd = (const uint8_t*)offsets + 2;
    args.offsets = &odd;
    assert(pq::write_error(args, false).find("not aligned to 4") != std::string::npos);
    const uint32_t strings[1] = {OXH_PARQUET_LIST | OXH_CSV_STRING};
    args.types = strings;
    assert(pq::write_error(args, false).find("list of element type 4") != std::string::npos);
    printf("ok\n");
    return 0;
}
