// tests/native/parquet_inflate_host_test.cpp -- what parquet_read_host.hpp adds for OXH_PARQUET_INFLATE, on the CPU:
// which codecs the footer planner accepts with and without the flag, the flag's own check, the bound on what a
// compressed page may claim, the image's plan and a compressed V1 page's levels once their length is known. Also what
// a sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"
#include "../../oxen_amd/csrc/parquet_read_host.hpp"

namespace pq = oxh::parquet;
namespace pr = oxh::pqr;

// The footer of a file of one REQUIRED INT64 column and one row group of 10 rows whose chunk names `codec`.
static pr::Footer footer_with(int32_t codec, bool inflate) {
    pq::Thrift t;
    t.i32(1, 1);
    t.list(2, pq::kTStruct, 2);
    t.begin(), t.binary(4, "schema", 6), t.i32(5, 1), t.end();
    t.begin(), t.i32(1, pr::kInt64), t.i32(3, 0), t.binary(4, "x", 1), t.end();
    t.i64(3, 10);
    t.list(4, pq::kTStruct, 1);
    t.begin();
    t.list(1, pq::kTStruct, 1);
    t.begin(), t.begin(3), t.i32(4, codec), t.i64(5, 10), t.i64(7, 100), t.i64(9, 4), t.end(), t.end();
    t.i64(3, 10);
    t.end();
    t.out.push_back(0);
    return pr::read_footer(t.out.data(), t.out.size(), 104, 104 + t.out.size() + 8, inflate);
}

int main() {
    for (int inflate = 0; inflate < 2; ++inflate) {
        const pr::Footer plain = footer_with(0, inflate);
        assert(plain.error.empty() && plain.chunks.size() == 1 && plain.chunks[0].codec == pr::kCodecNone && plain.chunks[0].bytes == 100);
        const pr::Footer snappy = footer_with(1, inflate);
        assert(snappy.error.empty() == (inflate == 1) && (inflate == 0 || snappy.chunks[0].codec == pr::kCodecSnappy));
        assert(inflate == 1 || snappy.error.find("column 'x': compression codec 1") != std::string::npos);
        for (int32_t codec : {2, 3, 4, 5, 6, 7})
            assert(footer_with(codec, inflate).error.find("compression codec " + std::to_string(codec)) != std::string::npos);
    }
    void* out = nullptr;
    uint64_t stats[8];
    const uint8_t byte = 0;
    assert(pr::open_error(&byte, 1, 0, &out, stats).empty() && pr::open_error(&byte, 1, OXH_PARQUET_INFLATE, &out, stats).empty());
    assert(pr::open_error(&byte, 1, 1, &out, stats) == "unknown flags" && pr::open_error(&byte, 1, 3, &out, stats) == "unknown flags");
    // 64 bytes from a 3-byte copy is the most a stream gives
    assert(pr::inflated_size_plausible(0, 32) && !pr::inflated_size_plausible(0, 33) && pr::inflated_size_plausible(100, 2232) &&
           !pr::inflated_size_plausible(100, 2233) && pr::inflated_size_plausible(0x7FFFFFFF, 0x7FFFFFFF));
    // the image: compressed pages only, in table order, on a 16-byte grid; stored levels are not the stream's
    std::vector<pr::PageRec> recs(4);
    recs[0] = pr::PageRec{4, 100, 0, 10, 0, 0, 0, 0, 0, 100, 0};
    recs[1] = pr::PageRec{200, 1000, 0, 10, 0, 0, 0, 0, pr::kPageInImage | pr::kPageLevelsLater, 50, 0};
    recs[2] = pr::PageRec{300, 33, 3, 10, 0, 0, 6, 6, pr::kPageInImage, 20, 6};
    recs[3] = pr::PageRec{400, 7, 2, 10, 0, 0, 0, 0, pr::kPageInImage, 9, 0};
    pr::ImagePlan plan = pr::plan_image(recs);
    assert(plan.implausible == ~0ull && plan.pages == 3 && plan.bytes == 1008 + 48 + 16 && plan.places[1] == 0 && plan.places[2] == 1008 && plan.places[3] == 1056);
    recs[2].body_size = 6 + 22 * 14 + 33;  // one more than 14 compressed bytes give
    assert(pr::plan_image(recs).implausible == 2);
    recs[2].body_size = 33, recs[2].stored = 21;  // more levels than the page has bytes in the file
    assert(pr::plan_image(recs).implausible == 2);
    pr::finish_v1_levels(recs[1], 996);
    assert(recs[1].def_at == 4 && recs[1].def_bytes == 996 && recs[1].values_at == 1000 && recs[1].flags == pr::kPageInImage);
    pr::finish_v1_levels(recs[1], 997);  // the levels leave the body: column_pages refuses the page
    assert(recs[1].values_at == ~0u);
    printf("ok\n");
    return 0;
}
