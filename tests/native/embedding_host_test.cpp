// tests/native/embedding_host_test.cpp -- the host-only pieces of oxh_embedding_* in a program of their own
// (embedding_host.hpp): the order key on hand-worked floats -- the code the kernel runs -- with its monotony and
// the unreachable null key, the argument checks in the header's order, the host forms' offset validation, the
// mean's partition, the page arithmetic and the staging plan. No HIP and no library: g++ -std=c++17 (add
// -fsanitize=address,undefined for a sanitizer run). Prints "ok" and exits 0, or says what failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../oxen_amd/csrc/embedding_host.hpp"

using namespace oxh;
namespace emb = oxh::embedding;

static int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static bool says(const std::string& got, const char* part) { return got.find(part) != std::string::npos; }

static uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static uint32_t key(float f) { return emb::order_key(bits_of(f)); }

static void order_keys() {
    EXPECT(OXH_EMB_FIXED == 0 && OXH_EMB_LIST32 == 1 && OXH_EMB_LIST64 == 2);
    // hand-worked: word(+1.0) = 0x3F800000 | 0x80000000 = 0xBF800000, its NOT 0x407FFFFF
    EXPECT(key(1.0f) == 0x407FFFFFu);
    EXPECT(key(0.0f) == 0x7FFFFFFFu && key(-0.0f) == 0x7FFFFFFFu);       // word(0) = 0x80000000; -0.0 is +0.0
    EXPECT(key(-1.0f) == 0xBF800000u);                                  // word(-1.0) = ~0xBF800000 = 0x407FFFFF
    const float inf = std::numeric_limits<float>::infinity();
    EXPECT(key(inf) == 0x007FFFFFu && key(-inf) == 0xFF800000u);
    // every NaN, whatever its sign or payload, is the one NaN above +inf: word 0xFFC00000, key 0x003FFFFF
    EXPECT(emb::order_key(0x7FC00000u) == 0x003FFFFFu && emb::order_key(0xFFC00000u) == 0x003FFFFFu);
    EXPECT(emb::order_key(0x7F800001u) == 0x003FFFFFu && emb::order_key(0xFFFFFFFFu) == 0x003FFFFFu);
    const float denorm = std::numeric_limits<float>::denorm_min();     // bits 1
    EXPECT(key(denorm) == 0x7FFFFFFEu && key(-denorm) == 0x80000001u);  // word(-denorm) = ~0x80000001 = 0x7FFFFFFE
    // strictly monotone: a larger similarity has a smaller key; NaN in front of all
    const float ladder[] = {inf, 2.0f, 1.0f, 0.70710677f, std::numeric_limits<float>::min(), denorm, 0.0f, -denorm,
                            -std::numeric_limits<float>::min(), -0.5f, -1.0f, -inf};
    uint32_t before = emb::order_key(0x7FC00000u);
    for (float f : ladder) {
        EXPECT(before < key(f));
        before = key(f);
    }
    // the null key is after every valid key and is no valid row's: the largest valid key is -inf's
    EXPECT(before == 0xFF800000u && before < emb::kNullKey && emb::kNullKey == 0xFFFFFFFFu);
    for (uint64_t b = 0; b <= 0xFFFFFFFFull; b += 0x10001ull) EXPECT(emb::order_key((uint32_t)b) <= 0xFF800000u);
    EXPECT(emb::order_key(0xFF800000u) == 0xFF800000u && emb::order_key(0xFF7FFFFFu) == 0xFF7FFFFFu);
}

static void column_checks() {
    alignas(16) float values[12] = {};
    int32_t off32[4] = {2, 5, 8, 11};
    int64_t off64[4] = {0, 3, 6, 9};
    const uint8_t valid[1] = {0x7};
    emb::Column good{OXH_EMB_LIST32, 3, 3, values, off32, valid, 0};
    for (int host = 0; host < 2; ++host) {
        EXPECT(emb::column_error(good, host).empty());
        emb::Column c = good;
        c.layout = 3;
        EXPECT(says(emb::column_error(c, host), "unknown layout"));
        c.dim = 0;  // the layout comes first
        EXPECT(says(emb::column_error(c, host), "unknown layout"));
        c = good, c.dim = 0;
        EXPECT(says(emb::column_error(c, host), "dim is 0"));
        c.nrows = 0xFFFFFFFFull;  // dim comes before the rows
        EXPECT(says(emb::column_error(c, host), "dim is 0"));
        c = good, c.nrows = 0xFFFFFFFFull;
        EXPECT(says(emb::column_error(c, host), "2^32 - 2"));
        c = good, c.values = (const uint8_t*)values + 2;
        EXPECT(says(emb::column_error(c, host), "4-byte aligned"));
        c = good, c.values = values + 1;  // any multiple of 4 bytes is fine
        EXPECT(emb::column_error(c, host).empty());
        c = good, c.offsets = nullptr;
        EXPECT(says(emb::column_error(c, host), "without offsets"));
        c = good, c.layout = OXH_EMB_FIXED, c.offsets = nullptr;
        EXPECT(emb::column_error(c, host).empty());
        c.values = nullptr;
        EXPECT(says(emb::column_error(c, host), "no values"));
        c = good, c.nrows = 0, c.values = nullptr, c.offsets = nullptr;  // no rows: nothing else is looked at
        EXPECT(emb::column_error(c, host).empty());
        c = good, c.layout = OXH_EMB_LIST64, c.offsets = off64;
        EXPECT(emb::column_error(c, host).empty());
    }
    // the offsets are read by the host forms only
    int32_t down[4] = {2, 5, 4, 11}, negative[4] = {-1, 2, 5, 8}, flat[4] = {4, 4, 4, 4};
    emb::Column c = good;
    c.offsets = down;
    EXPECT(emb::column_error(c, false).empty() && says(emb::column_error(c, true), "decrease at row 1"));
    c.offsets = negative;
    EXPECT(emb::column_error(c, false).empty() && says(emb::column_error(c, true), "negative"));
    c.offsets = off32, c.values = nullptr;
    EXPECT(says(emb::column_error(c, true), "elements but no values") && says(emb::column_error(c, false), "no values"));
    c.offsets = flat;  // an empty span needs no values in the host form
    EXPECT(emb::column_error(c, true).empty());
}

static void entry_checks() {
    alignas(16) float values[6] = {};
    float out[3], query[3] = {};
    uint32_t idx[2] = {0, 1}, keys[2], perm[2];
    uint8_t bitmap[1];
    uint64_t stats[4];
    const uint8_t valid[1] = {0x3};
    const emb::Column col{OXH_EMB_FIXED, 2, 3, values, nullptr, nullptr, 0};
    {
        emb::MeanArgs a{col, idx, 2, out, stats};
        EXPECT(emb::mean_error(a, true).empty() && emb::mean_error(a, false).empty());
        a.col.layout = 9, a.stats4 = nullptr;  // the column comes first
        EXPECT(says(emb::mean_error(a, false), "unknown layout"));
        a = {col, nullptr, 2, out, stats};
        EXPECT(says(emb::mean_error(a, false), "idx is NULL"));
        a = {col, idx, 2, nullptr, stats};
        EXPECT(says(emb::mean_error(a, false), "out is NULL"));
        a = {col, idx, 2, out, nullptr};
        EXPECT(says(emb::mean_error(a, true), "stats4 is NULL"));
        a = {col, nullptr, 0, nullptr, stats};  // no indices: nothing to read or write
        EXPECT(emb::mean_error(a, true).empty());
        uint32_t past[2] = {1, 2};
        a = {col, past, 2, out, stats};
        EXPECT(says(emb::mean_error(a, true), "idx[1] = 2 is not a row of 2") && emb::mean_error(a, false).empty());
        a = {col, idx, 0xFFFFFFFFull, out, stats};
        EXPECT(says(emb::mean_error(a, false), "2^32 - 2 indices"));
    }
    {
        emb::SimilarityArgs a{col, query, out, nullptr, keys, perm, stats};
        EXPECT(emb::similarity_error(a, true).empty());
        a.order_key = nullptr;
        EXPECT(says(emb::similarity_error(a, false), "perm needs order_key"));
        a.perm = nullptr;
        EXPECT(emb::similarity_error(a, false).empty());
        a = {col, nullptr, out, nullptr, keys, perm, stats};
        EXPECT(says(emb::similarity_error(a, false), "query is NULL"));
        a = {col, query, nullptr, nullptr, keys, perm, stats};
        EXPECT(says(emb::similarity_error(a, false), "sim is NULL"));
        a = {col, query, out, nullptr, keys, perm, stats};
        a.col.validity = valid;
        EXPECT(says(emb::similarity_error(a, false), "sim_validity is NULL"));
        a.sim_validity = bitmap;
        EXPECT(emb::similarity_error(a, false).empty());
        a.stats4 = nullptr;
        EXPECT(says(emb::similarity_error(a, false), "stats4 is NULL"));
        a = {col, nullptr, nullptr, nullptr, nullptr, nullptr, stats};
        a.col.nrows = 0;  // no rows: only stats4 is needed
        EXPECT(emb::similarity_error(a, true).empty());
    }
    {
        uint32_t some[2] = {1, OXH_TAKE_NULL};
        emb::TakeArgs a{col, some, 2, out, bitmap, stats};
        EXPECT(emb::take_error(a, true).empty() && emb::take_error(a, false).empty());
        a.idx = nullptr;
        EXPECT(says(emb::take_error(a, false), "idx, out_values or out_validity is NULL"));
        a = {col, some, 2, out, nullptr, stats};
        EXPECT(says(emb::take_error(a, false), "idx, out_values or out_validity is NULL"));
        a = {col, some, 2, out, bitmap, nullptr};
        EXPECT(says(emb::take_error(a, false), "stats4 is NULL"));
        uint32_t past[2] = {2, 0};
        a = {col, past, 2, out, bitmap, stats};
        EXPECT(says(emb::take_error(a, true), "idx[0] = 2 is neither absent nor a row of 2") && emb::take_error(a, false).empty());
        a = {col, nullptr, 0, nullptr, nullptr, stats};
        EXPECT(emb::take_error(a, true).empty());
    }
}

static void partition() {
    EXPECT(emb::kMeanChunk == 64 && emb::kMeanMaxGroups == 1024);
    EXPECT(emb::mean_groups(0) == 1 && emb::mean_groups(1) == 1 && emb::mean_groups(64) == 1 && emb::mean_groups(65) == 2);
    EXPECT(emb::mean_groups(64 * 1024) == 1024 && emb::mean_groups(64 * 1024 + 1) == 1024 && emb::mean_groups(0xFFFFFFFEull) == 1024);
    EXPECT(emb::mean_lanes(1) == 1 && emb::mean_lanes(2) == 2 && emb::mean_lanes(3) == 4 && emb::mean_lanes(8) == 8);
    EXPECT(emb::mean_lanes(255) == 256 && emb::mean_lanes(256) == 256 && emb::mean_lanes(257) == 256 && emb::mean_lanes(4097) == 256);
    EXPECT(emb::mean_lease_bytes(1, 768) == 256 + 3072 && emb::mean_lease_bytes(65, 3) == 256 + 256);
}

static void pages() {
    auto is = [](emb::Page p, uint64_t first, uint64_t count) { return p.first == first && p.count == count; };
    EXPECT(is(emb::page_of(1000, 100, 1), 0, 100) && is(emb::page_of(1000, 100, 0), 0, 100));  // page 0 means 1
    EXPECT(is(emb::page_of(1000, 100, 10), 900, 100) && is(emb::page_of(1000, 100, 11), 1000, 0));
    EXPECT(is(emb::page_of(1001, 100, 11), 1000, 1) && is(emb::page_of(1001, 100, 12), 1001, 0));
    EXPECT(is(emb::page_of(7, 100, 1), 0, 7) && is(emb::page_of(0, 100, 1), 0, 0) && is(emb::page_of(7, 0, 3), 7, 0));
    EXPECT(is(emb::page_of(7, 3, ~0ull), 7, 0) && is(emb::page_of(0xFFFFFFFEull, ~0ull, 2), 0xFFFFFFFEull, 0));  // no overflow
}

static void staging() {
    // a list column of 5 rows whose first offset is not 0, rows 1..3 staged: their offsets, their elements at
    // the caller's phase within 16 bytes, and the validity byte that holds their bits
    alignas(16) float values[32] = {};
    int32_t off[6] = {3, 6, 9, 12, 15, 18};
    const uint8_t valid[2] = {0xFF, 0xFF};
    const emb::Column c{OXH_EMB_LIST32, 5, 3, values, off, valid, 6};
    emb::HostPlan plan;
    const int64_t front = plan.add(nullptr, 20);
    EXPECT(front == 0 && plan.total == 32);
    plan.add_column(c, 1, 4);
    EXPECT(plan.row_lo == 1 && plan.row_hi == 4 && plan.elem_lo == 6 && plan.elem_hi == 15);
    EXPECT(plan.pieces[plan.offsets].src == (const void*)(off + 1) && plan.pieces[plan.offsets].bytes == 16 && plan.pieces[plan.offsets].at == 32);
    EXPECT(plan.pieces[plan.values].src == (const void*)(values + 6) && plan.pieces[plan.values].bytes == 36);
    EXPECT(plan.pieces[plan.values].at == 48 + 8);          // values + 6 floats is 8 bytes past a 16-byte boundary
    EXPECT(plan.pieces[plan.values].at % 16 == (uintptr_t)(values + 6) % 16);
    EXPECT(plan.nbit == 7 && plan.pieces[plan.validity].src == (const void*)valid && plan.pieces[plan.validity].bytes == 2);
    EXPECT(plan.pieces[plan.validity].at == 48 + 48 && plan.total == 48 + 48 + 16);
    for (const emb::Piece& p : plan.pieces) EXPECT(p.at + p.bytes <= plan.total);
    uint8_t block[8];
    EXPECT(plan.at(block, -1) == nullptr && plan.at(block, front) == block);
    // the fixed layout: rows [2, 5) of dim 3 are elements [6, 15); no offsets, no validity
    emb::HostPlan fixed;
    fixed.add_column(emb::Column{OXH_EMB_FIXED, 5, 3, values + 1, nullptr, nullptr, 0}, 2, 5);
    EXPECT(fixed.offsets == -1 && fixed.validity == -1 && fixed.elem_lo == 6 && fixed.elem_hi == 15);
    EXPECT(fixed.pieces[fixed.values].src == (const void*)(values + 7) && fixed.pieces[fixed.values].at == 12 && fixed.total == 48);
    emb::HostPlan none;
    none.add_column(c, 0, 0);
    EXPECT(none.pieces.empty() && none.total == 0 && none.values == -1);
}

int main() {
    order_keys();
    column_checks();
    entry_checks();
    partition();
    pages();
    staging();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
