// tests/native/parquet_host_test.cpp -- parquet_host.hpp on the CPU: the planner over hand-made tile tables (page and
// row-group cuts, places, the booleans' carried bits, offsets, refusals, an empty frame whose footer it prints for
// tests/test_parquet_write_cpu.py to decode) and the zeros of the statistics. Also what a sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"

namespace pq = oxh::parquet;

static pq::Tile tile(uint32_t valid, uint64_t bytes, uint64_t lo = 0, uint64_t hi = 0, bool has = false) {
    pq::Tile t{};
    t.valid = valid, t.value_bytes = bytes, t.min = lo, t.max = hi, t.has_minmax = has;
    return t;
}

int main() {
    // statistics: a NaN-only tile carries nothing; whichever zeros the tiles kept, the min is -0.0 and the max +0.0
    const uint64_t minus_zero = 1ull << 63;
    pq::MinMax d;
    d.fold(tile(5, 40), OXH_CSV_FLOAT64), d.fold(tile(5, 40, 0, minus_zero, true), OXH_CSV_FLOAT64), d.finish(OXH_CSV_FLOAT64);
    assert(d.has && d.min == minus_zero && d.max == 0);
    // the planner: 2 500 rows, three columns, groups of 2 048 rows, pages of 4 096 bytes
    const uint32_t types[3] = {OXH_CSV_INT64, OXH_CSV_BOOL, OXH_CSV_STRING};
    const uint8_t names[] = "idflagtext";
    const uint64_t name_offsets[4] = {0, 2, 6, 10};
    const uint32_t rows[3] = {1024, 1024, 452};
    std::vector<pq::Tile> tiles;
    for (int k = 0; k < 3; ++k) {
        tiles.push_back(tile(rows[k], 8ull * rows[k], (uint64_t)(-10ll * k), 100 + k, true));
        tiles.push_back(tile(rows[k] - 10, rows[k] - 10, 0x2B));  // the last valid rows: 1 1 0 1 0 1 0, newest first
        tiles.push_back(tile(rows[k] - (k == 1), 5000 + k));
    }
    const pq::Plan p = pq::make_plan(2500, 3, types, names, name_offsets, 2048, 4096, tiles.data());
    assert(p.error.empty() && p.row_groups == 2 && p.pages.size() == 8 && p.null_cells == 31);
    uint64_t at = 4;
    for (const pq::Page& g : p.pages) {
        assert(g.file_at == at && g.head_len < 64 && g.head_src + g.head_len <= p.blob.size());
        at += g.head_len + g.level_bytes + g.values_bytes;
    }
    assert(at + p.footer.size() == p.out_bytes);
    assert(p.pages[2].col == 1 && p.pages[2].rows == 2048 && p.pages[2].nvalid == 2028 && p.pages[2].level_bytes == 256 && p.pages[2].values_bytes == 254);
    assert(p.places[1 * 3 + 1].page == 2 && p.places[1 * 3 + 1].rank_base == 1014 && p.places[1 * 3 + 1].byte_base == 0x35 && p.places[1].byte_base == 0);
    assert(p.places[1 * 3 + 2].page == 4 && p.places[1 * 3 + 2].byte_base == 0 && p.pages[4].level_bytes == 128 && p.pages[3].level_bytes == 0);
    assert(p.pages[5].tile0 == 2 && p.pages[5].row0 == 2048 && p.pages[5].rows == 452);
    // greedy: string tiles of 1 000 bytes share a page until levels plus values reach the budget
    std::vector<pq::Tile> small(9, tile(1024, 1000));
    const pq::Plan q = pq::make_plan(9 * 1024, 1, types + 2, names, name_offsets, 0, 4096, small.data());
    assert(q.error.empty() && q.row_groups == 1 && q.pages.size() == 2 && q.pages[0].rows == 5 * 1024 && q.places[4].byte_base == 4000 && q.places[5].page == 1);
    const pq::Tile huge = tile(1024, 0x7FFFFFFFull), wrong = tile(1025, 8200);
    assert(!pq::make_plan(1024, 1, types + 2, names, name_offsets, 0, 0, &huge).error.empty() && !pq::make_plan(1024, 1, types, names, name_offsets, 0, 0, &wrong).error.empty());
    std::vector<pq::Tile> many(32768, tile(1024, 1024));
    assert(pq::make_plan(32768 * 1024, 1, types + 1, names, name_offsets, 1024, 0, many.data()).error.find("ordinal") != std::string::npos);
    const pq::Plan e = pq::make_plan(0, 3, types, names, name_offsets, 0, 0, nullptr);
    assert(e.error.empty() && e.pages.empty() && e.row_groups == 0 && e.out_bytes == 4 + e.footer.size());
    printf("empty ");
    for (uint8_t x : e.footer) printf("%02x", x);
    printf("\nok\n");
    return 0;
}
