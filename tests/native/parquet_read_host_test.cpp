// tests/native/parquet_read_host_test.cpp -- parquet_bits.hpp and parquet_read_host.hpp on the CPU: the Thrift reader
// on every truncation of a footer and of a page header, the hybrid's run walk on streams that end early or overrun,
// the extraction of every value at every width 1 .. 32 against a shift-and-mask over a 128-bit integer, and the
// footer planner on the empty file and on a planned file of the writer's planner (parquet_host.hpp), with its
// refusals. This is where widths above those of the fixtures and malformed streams are covered. Also what a
// sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"
#include "../../oxen_amd/csrc/parquet_read_host.hpp"

namespace pq = oxh::parquet;
namespace pr = oxh::pqr;

static uint64_t mix(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The footer of a file of the writer's planner: "PAR1" is not part of it, the footer is its last bytes.
static pr::Footer footer_of(const pq::Plan& p, uint64_t len_change = 0) {
    const uint64_t meta = p.footer.size() - 8, at = p.out_bytes - p.footer.size();
    return pr::read_footer(p.footer.data(), meta - len_change, at, p.out_bytes);
}

int main() {
    // varints: every length, the longest, one too long, one cut short
    {
        const uint8_t max64[10] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x01};
        pr::Span s{max64, 10, 0, false};
        assert(pr::varint(s) == ~0ull && !s.bad && s.at == 10);
        const uint8_t long11[11] = {0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x01};
        pr::Span t{long11, 11, 0, false};
        (void)pr::varint(t);
        assert(t.bad);
        pr::Span u{max64, 9, 0, false};
        (void)pr::varint(u);
        assert(u.bad);
        assert(pr::zigzag(0) == 0 && pr::zigzag(1) == -1 && pr::zigzag(2) == 1 && pr::zigzag(~0ull) == INT64_MIN);
    }
    // value k of width w against a shift-and-mask over the run as one 128-bit integer
    uint64_t seed = 7;
    for (uint32_t w = 1; w <= 32; ++w) {
        uint8_t run[16];
        for (int round = 0; round < 8; ++round) {
            for (uint8_t& b : run) b = (uint8_t)mix(seed);
            unsigned __int128 all = 0;
            for (int b = 15; b >= 0; --b) all = (all << 8) | run[b];
            const unsigned __int128 mask = ((unsigned __int128)1 << w) - 1;
            for (uint64_t k = 0; (k + 1) * w <= 128; ++k) assert(pr::extract(run, 16, k, w) == (uint32_t)((all >> (k * w)) & mask));
            // bytes past `avail` read as zeros and are never touched (the sanitizer build proves the second half)
            const uint64_t cut = 1 + mix(seed) % 15;
            for (uint64_t k = 0; (k + 1) * w <= 128; ++k) {
                const unsigned __int128 kept = all & (((unsigned __int128)1 << (8 * cut)) - 1);
                assert(pr::extract(run, cut, k, w) == (uint32_t)((kept >> (k * w)) & mask));
            }
        }
        assert(pr::extract(run, 16, 3, 0) == 0);
    }
    // the run walk: an RLE run, a bit-packed run, a last group cut short by its writer, streams that end early
    {
        const uint8_t rle[] = {0x0A, 0x05, 0x03, 0xAB, 0xCD};  // 5 x value 5 at width 3, then one group of 8 at width 3 ...
        pr::Span s{rle, sizeof rle, 0, false};
        pr::Run r;
        assert(pr::next_run(s, 3, 100, r) && !r.packed && r.count == 5 && r.value == 5);
        assert(!pr::next_run(s, 3, 100, r) && s.bad);  // ... whose 3 bytes are not there when 8 values are wanted
        pr::Span t{rle, sizeof rle, 2, false};
        assert(pr::next_run(t, 3, 5, r) && r.packed && r.count == 8 && r.avail == 2 && pr::extract(r.body, r.avail, 4, 3) == ((0xCDABu >> 12) & 7));
        const uint8_t wide[] = {0x02, 0x08};                   // 1 x value 8 at width 3: it does not fit
        pr::Span u{wide, 2, 0, false};
        assert(!pr::next_run(u, 3, 1, r) && u.bad);
        const uint8_t empty[] = {0x00, 0x01};                  // an empty run would never end the walk
        pr::Span v{empty, 2, 0, false};
        assert(!pr::next_run(v, 1, 1, r));
        const uint8_t huge[] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x01, 0x55};  // 2^60 groups: clamped, not multiplied over
        pr::Span x{huge, sizeof huge, 0, false};
        assert(pr::next_run(x, 1, 8, r) && r.packed && r.avail == 1 && r.count == pr::kMaxGroups * 8);
        for (uint64_t cut = 0; cut < sizeof rle; ++cut) {      // every truncation ends in `bad`, never past the span
            pr::Span c{rle, cut, 0, false};
            uint64_t got = 0;
            while (got < 13 && pr::next_run(c, 3, 13 - got, r)) got += r.count;
            assert(got < 13 && (c.bad || got == 5));
        }
    }
    // a page header as the writer's planner makes it, whole and on every truncation
    const uint32_t types[3] = {OXH_CSV_INT64, OXH_CSV_BOOL, OXH_CSV_STRING};
    const uint8_t names[] = "idflagtext";
    const uint64_t name_offsets[4] = {0, 2, 6, 10};
    std::vector<pq::Tile> tiles;
    for (int t = 0; t < 3; ++t)
        for (int c = 0; c < 3; ++c) {
            pq::Tile tl{};
            tl.valid = 1000, tl.value_bytes = c == 0 ? 8000 : c == 1 ? 1000 : 9000;
            tiles.push_back(tl);
        }
    const pq::Plan p = pq::make_plan(3 * 1024, 3, types, names, name_offsets, 2048, 4096, tiles.data());
    assert(p.error.empty());
    {
        const pq::Page& g = p.pages[0];
        pr::Span s{p.blob.data() + g.head_src, g.head_len, 0, false};
        pr::PageInfo h;
        uint64_t st[pr::kSkipDepth];
        assert(pr::page_header(s, h, st) && h.type == pr::kPageData && h.num_values == (int32_t)g.rows && h.encoding == pr::kEncPlain && h.def_enc == pr::kEncRle);
        assert(h.csize == h.usize && (uint64_t)h.csize == g.head_len - s.at + g.level_bytes + g.values_bytes);
        const uint64_t header = s.at;
        for (uint64_t cut = 0; cut < header; ++cut) {
            pr::Span c{p.blob.data() + g.head_src, cut, 0, false};
            assert(!pr::page_header(c, h, st) && c.bad && c.at <= cut);
        }
    }
    // the footer planner: the planned file, every truncation of its footer, and its refusals
    {
        const pr::Footer f = footer_of(p);
        assert(f.error.empty() && f.nrows == 3 * 1024 && f.leaves.size() == 3 && f.group_rows.size() == 2 && f.chunks.size() == 6);
        assert(f.leaves[0].name == "id" && f.leaves[0].physical == pr::kInt64 && !f.leaves[0].required && f.leaves[2].physical == pr::kByteArray);
        assert(f.chunks[0].at == 4 && f.chunks[0].num_values == 2048 && f.chunks[3].num_values == 1024 && f.chunks[1].at == 4 + f.chunks[0].bytes);
        for (uint64_t cut = 1; cut < p.footer.size() - 8; ++cut) assert(!footer_of(p, cut).error.empty());
        std::vector<uint8_t> meta(p.footer.begin(), p.footer.end() - 8);
        const uint64_t at = p.out_bytes - p.footer.size();
        assert(!pr::read_footer(meta.data(), meta.size(), at - 1, p.out_bytes).error.empty());  // the last chunk ends behind the pages
        uint64_t where = 0, len = 0;
        const uint8_t* tail = p.footer.data() + p.footer.size() - 8;
        assert(pr::footer_place((const uint8_t*)"PAR1", tail, p.out_bytes, where, len).empty() && where == at && len == meta.size());
        assert(!pr::footer_place((const uint8_t*)"PAR2", tail, p.out_bytes, where, len).empty());
        assert(pr::footer_place((const uint8_t*)"PARE", tail, p.out_bytes, where, len).find("encrypted") != std::string::npos);
        assert(!pr::footer_place((const uint8_t*)"PAR1", tail, meta.size() + 11, where, len).empty());
        assert(!pr::footer_place((const uint8_t*)"PAR1", tail, 11, where, len).empty());
    }
    // a nested schema: root { g { x } } and root { g { } x } -- a group is named whether or not the root's count fits
    for (int shape = 0; shape < 2; ++shape) {
        pq::Thrift t;
        t.i32(1, 1);
        t.list(2, pq::kTStruct, 3);
        t.begin(), t.binary(4, "schema", 6), t.i32(5, shape ? 2 : 1), t.end();
        t.begin(), t.i32(3, 1), t.binary(4, "g", 1), t.i32(5, 1), t.end();
        t.begin(), t.i32(1, 2), t.i32(3, 1), t.binary(4, "x", 1), t.end();
        t.i64(3, 0);
        t.list(4, pq::kTStruct, 0);
        t.out.push_back(0);
        const pr::Footer nested = pr::read_footer(t.out.data(), t.out.size(), 4, 4 + t.out.size() + 8);
        assert(nested.error.find("column 'g' is a nested field") != std::string::npos);
    }
    {   // a field of type 0 is no field: the span goes bad, it is not walked as a struct
        const uint8_t zero_type[] = {0x10, 0x15, 0x02, 0x00, 0x00};
        pr::Span s{zero_type, sizeof zero_type, 0, false};
        uint64_t st[pr::kSkipDepth];
        pr::PageInfo h;
        assert(!pr::page_header(s, h, st) && s.bad);
    }
    const pq::Plan e = pq::make_plan(0, 3, types, names, name_offsets, 0, 0, nullptr);
    const pr::Footer none = footer_of(e);
    assert(e.error.empty() && none.error.empty() && none.nrows == 0 && none.leaves.size() == 3 && none.chunks.empty() && none.leaves[1].physical == pr::kBoolean);
    const std::vector<pr::ChunkDesc> no_chunks;
    const pr::ColumnPages cp = pr::column_pages(none, 0, no_chunks, {}, {});
    assert(cp.cause.empty() && cp.data.empty() && cp.words == 0);
    assert(pr::type_fits(pr::kInt32, OXH_CSV_INT64) && pr::type_fits(pr::kFloat, OXH_CSV_FLOAT32) && !pr::type_fits(pr::kInt64, OXH_CSV_INT32) &&
           !pr::type_fits(pr::kInt96, 0) && !pr::native_type(pr::kFixedLen));
    printf("ok\n");
    return 0;
}
