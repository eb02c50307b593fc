// tests/native/concat_columns_host_test.cpp -- the host-only pieces of oxh_concat_columns_* (oxen_amd/csrc/
// concat_columns_host.hpp, columns.hpp) in a program of their own: the argument checks in the header's order,
// the prefix table of rows, the bit streams, the sizes, the spans and the item lists (pieces on the
// destination's 16-byte grid), and the host form's staging plan (only the taken ranges). No HIP and no
// library: g++ -std=c++17 (add -fsanitize=address,undefined for a sanitizer run). Prints "ok" and exits 0, or
// says what failed and exits 1.
#include <cstdio>
#include <cstring>

#include "../../oxen_amd/csrc/concat_columns_host.hpp"

using namespace oxh;

static int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static bool says(const std::string& got, const char* part) { return got.find(part) != std::string::npos; }

// Two parts of three columns -- Int32, Boolean, BYTES32 -- of 3 and 2 rows; rows [1, 3) of the first and
// [0, 2) of the second are taken: 4 output rows.
struct Call {
    int32_t ints0[3] = {1, 2, 3}, ints1[2] = {4, 5};
    uint8_t bools0[1] = {0b101}, bools1[1] = {0b10};
    char text0[7] = "abcdef", text1[4] = "xyz";
    int32_t off0[4] = {1, 3, 3, 6}, off1[3] = {0, 1, 3};
    uint8_t valid0[1] = {0b011};
    uint32_t kinds[3] = {OXH_COL_FIXED4, OXH_COL_BOOL, OXH_COL_BYTES32};
    const void* values[6] = {ints0, bools0, text0, ints1, bools1, text1};
    const void* offsets[6] = {nullptr, nullptr, off0, nullptr, nullptr, off1};
    const uint8_t* validity[6] = {nullptr, valid0, nullptr, nullptr, nullptr, nullptr};
    uint64_t bits[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t rows[2] = {3, 2};
    uint64_t first[2] = {1, 0}, count[2] = {2, 2};
    uint64_t capacity[3] = {0, 0, 64};
    alignas(16) uint8_t v0[16], v1[8], v2[64], n0[8], n1[8], n2[8];
    int32_t o2[5];
    void* out_values[3] = {v0, v1, v2};
    void* out_offsets[3] = {nullptr, nullptr, o2};
    uint8_t* out_validity[3] = {n0, n1, n2};
    uint64_t value_bytes[3] = {7, 7, 7};
    uint32_t written = 7;
    concat::Args a{2, 3, kinds, values, offsets, validity, bits, rows, first, count, capacity, out_values, out_offsets,
                   out_validity, value_bytes, &written};
};

static void arguments() {
    for (const bool host : {true, false}) {
        Call c;
        EXPECT(concat::argument_error(c.a, host).empty());
        {
            Call d;  // the sizes-only call: value_capacity is not looked at
            d.a.out_values = nullptr, d.a.out_offsets = nullptr, d.a.out_validity = nullptr, d.a.value_capacity = nullptr;
            EXPECT(concat::argument_error(d.a, host).empty() && concat::sizes_only(d.a));
        }
        {
            Call d;  // whole parts: first is not read
            d.a.count = nullptr, d.a.first = nullptr;
            EXPECT(concat::argument_error(d.a, host).empty() && concat::row_table(d.a).back() == 5);
        }
#define BAD(change, part)                                     \
    do {                                                      \
        Call d;                                               \
        change;                                               \
        EXPECT(says(concat::argument_error(d.a, host), part)); \
    } while (0)
        BAD(d.a.kinds = nullptr, "is NULL");
        BAD(d.a.values = nullptr, "is NULL");
        BAD(d.a.offsets = nullptr, "is NULL");
        BAD(d.a.validity = nullptr, "is NULL");
        BAD(d.a.bit_offsets = nullptr, "is NULL");
        BAD(d.a.part_rows = nullptr, "is NULL");
        BAD(d.a.first = nullptr, "is NULL");
        BAD(d.a.nparts = 0, "is 0");
        BAD(d.a.ncols = 0, "is 0");
        BAD(d.a.nparts = OXH_CONCAT_MAX_PARTS + 1, "OXH_CONCAT_MAX_PARTS");
        BAD(d.kinds[1] = 3, "unknown kind 3");
        BAD(d.count[0] = 3, "part 0: first + count");
        BAD(d.first[1] = 3, "part 1: first + count");
        BAD((d.first[0] = ~0ull, d.count[0] = 2), "part 0: first + count");  // no wrap-around
        BAD((d.rows[1] = concat::kMaxRows + 1), "part 1 has more than 2^32 - 2 rows");
        BAD((d.rows[0] = d.rows[1] = concat::kMaxRows, d.first[0] = 0, d.count[0] = concat::kMaxRows, d.count[1] = 1), "output rows");
        BAD(d.a.value_bytes = nullptr, "value_bytes or written");
        BAD(d.a.written = nullptr, "value_bytes or written");
        BAD(d.offsets[5] = nullptr, "part 1 column 2 is a byte column without offsets");
        BAD(d.values[3] = nullptr, "part 1 column 0 has no values");
        BAD(d.values[1] = nullptr, "part 0 column 1 has no values");
        BAD(d.a.out_values = nullptr, "some of");
        BAD(d.a.value_capacity = nullptr, "value_capacity");
        BAD(d.out_offsets[2] = nullptr, "without out_offsets");
        BAD(d.out_validity[0] = nullptr, "no out_validity");
        BAD(d.out_values[1] = nullptr, "no out_values");
        BAD(d.out_values[2] = nullptr, "value_capacity but no out_values");
        // the order: each earlier check wins over each later one
        BAD((d.a.kinds = nullptr, d.a.nparts = 0), "is NULL");
        BAD((d.a.nparts = 0, d.kinds[0] = 3), "is 0");
        BAD((d.a.nparts = OXH_CONCAT_MAX_PARTS + 1, d.kinds[0] = 3), "OXH_CONCAT_MAX_PARTS");
        BAD((d.kinds[0] = 3, d.count[0] = 9), "unknown kind");
        BAD((d.count[0] = 9, d.rows[1] = concat::kMaxRows + 1), "first + count");
        BAD((d.rows[1] = concat::kMaxRows + 1, d.a.written = nullptr), "2^32 - 2 rows");
        BAD((d.a.written = nullptr, d.offsets[2] = nullptr), "value_bytes or written");
        BAD((d.offsets[2] = nullptr, d.values[0] = nullptr), "without offsets");
        BAD((d.values[0] = nullptr, d.a.out_values = nullptr), "no values");
        {
            Call d;  // a part none of whose rows are taken needs no arrays
            d.count[1] = 0, d.values[3] = d.values[4] = d.values[5] = nullptr, d.offsets[5] = nullptr;
            EXPECT(concat::argument_error(d.a, host).empty());
        }
    }
    // the device form only: the bit-packed outputs are written a word at a time
    {
        Call d;
        d.out_validity[2] = d.n2 + 4;
        EXPECT(says(concat::argument_error(d.a, false), "not 8-byte aligned") && concat::argument_error(d.a, true).empty());
        Call e;
        e.out_values[1] = e.v1 + 1;
        EXPECT(says(concat::argument_error(e.a, false), "not 8-byte aligned") && concat::argument_error(e.a, true).empty());
    }
    // the host form only: it reads the offsets of the taken range, and nothing outside it
    {
        Call d;
        d.off0[2] = 2;  // rows [1, 3) of part 0 read off0[1..3] = 3, 2, 6
        EXPECT(says(concat::argument_error(d.a, true), "part 0 column 2: offsets decrease at row 0") && concat::argument_error(d.a, false).empty());
        Call e;
        e.off0[0] = 9;  // outside the taken range
        EXPECT(concat::argument_error(e.a, true).empty());
        Call f;
        f.off1[0] = -1;
        EXPECT(says(concat::argument_error(f.a, true), "part 1 column 2: offsets[0] is negative"));
        Call g;
        g.values[5] = nullptr;
        EXPECT(says(concat::argument_error(g.a, true), "part 1 column 2 has bytes but no values") && concat::argument_error(g.a, false).empty());
        Call h;  // the output rules come before the host form's look at the offsets
        h.off0[2] = 2, h.out_validity[0] = nullptr;
        EXPECT(says(concat::argument_error(h.a, true), "no out_validity"));
    }
}

static void plan() {
    Call c;
    concat::Plan plan(c.a);
    EXPECT(plan.row_base == (std::vector<uint64_t>{0, 2, 4}) && plan.n == 4);
    EXPECT(plan.byte_cols == std::vector<uint32_t>{2} && plan.bool_cols == std::vector<uint32_t>{1} && plan.nstreams(c.a) == 4);
    EXPECT(plan.need[0] == 16 && plan.need[1] == 1);
    c.bits[2] = 5, c.bits[3] = 9;  // part 0's boolean column: values at bit 5, validity at bit 9
    plan.make_bits(c.a);
    EXPECT(plan.bits.size() == 8);
    EXPECT(plan.bits[0].p == nullptr && plan.bits[1].p == nullptr);            // column 0's validity: both parts all valid
    EXPECT(plan.bits[2].p == c.valid0 && plan.bits[2].bit == 10);              // column 1's validity of part 0, at its first row
    EXPECT(plan.bits[3].p == nullptr);
    EXPECT(plan.bits[6].p == c.bools0 && plan.bits[6].bit == 6 && plan.bits[7].p == c.bools1 && plan.bits[7].bit == 0);
    concat::host_spans(c.a, plan);
    EXPECT(plan.byte_span[0].lo == 3 && plan.byte_span[0].hi == 6 && plan.byte_span[1].lo == 0 && plan.byte_span[1].hi == 3);
    EXPECT(plan.make_sizes(c.a).empty() && plan.need[2] == 6 && !plan.bad_span && plan.fits(c.a));
    c.capacity[2] = 5;
    EXPECT(!plan.fits(c.a));
    plan.make_items(c.a, c.out_values, c.out_offsets);
    // spans: column 0 of both parts, the two rebases, then the two byte copies
    EXPECT(plan.spans.size() == 6 && plan.fixed_items.size() == 4 && plan.byte_items.size() == 2);
    EXPECT(plan.spans[0].src == (const uint8_t*)(c.ints0 + 1) && plan.spans[0].dst == c.v0 && plan.spans[0].n == 8 && plan.spans[0].mode == 0);
    EXPECT(plan.spans[1].src == (const uint8_t*)c.ints1 && plan.spans[1].dst == c.v0 + 8 && plan.spans[1].n == 8);
    EXPECT(plan.spans[2].mode == 4 && plan.spans[2].src == (const uint8_t*)(c.off0 + 1) && plan.spans[2].dst == (uint8_t*)c.o2 &&
           plan.spans[2].n == 2 && plan.spans[2].lo == 3 && plan.spans[2].hi == 6 && plan.spans[2].base == 0);
    EXPECT(plan.spans[3].mode == 4 && plan.spans[3].dst == (uint8_t*)(c.o2 + 2) && plan.spans[3].n == 3 && plan.spans[3].base == 3);  // and off[N]
    EXPECT(plan.spans[4].src == (const uint8_t*)c.text0 + 3 && plan.spans[4].dst == c.v2 && plan.spans[4].n == 3);
    EXPECT(plan.spans[5].src == (const uint8_t*)c.text1 && plan.spans[5].dst == c.v2 + 3 && plan.spans[5].n == 3);
    EXPECT(plan.byte_items[0].span == 4 && plan.byte_items[1].span == 5 && plan.byte_items[1].piece == 0);
    // an empty part in the middle brings nothing, and the last part WITH rows writes off[N]
    {
        Call d;
        d.count[1] = 0;
        concat::Plan q(d.a);
        concat::host_spans(d.a, q);
        EXPECT(q.make_sizes(d.a).empty() && q.need[2] == 3 && q.n == 2);
        q.make_items(d.a, d.out_values, d.out_offsets);
        EXPECT(q.spans.size() == 3 && q.spans[1].mode == 4 && q.spans[1].n == 3);
    }
    // a bad span holds no bytes and every offset of it is its base; BYTES32 above 2^31 - 1 bytes
    {
        Call d;
        concat::Plan q(d.a);
        q.byte_span = {{5, 2}, {0, 3}};
        EXPECT(q.make_sizes(d.a).empty() && q.bad_span && q.need[2] == 3);
        q.make_items(d.a, d.out_values, d.out_offsets);
        EXPECT(q.spans.size() == 5 && q.spans[2].lo == 0 && q.spans[2].hi == 0 && q.spans[3].base == 0 && q.spans[4].dst == d.v2);
        q.byte_span = {{-1, 2}, {0, 3}};
        EXPECT(q.make_sizes(d.a).empty() && q.bad_span && q.need[2] == 3);
        q.byte_span = {{0, 0x40000000}, {0, 0x40000000}};
        EXPECT(says(q.make_sizes(d.a), "OXH_COL_BYTES64"));
        q.byte_span = {{0, 0x40000000}, {1, 0x40000000}};
        EXPECT(q.make_sizes(d.a).empty() && q.need[2] == concat::kMaxBytes32);
        d.values[5] = nullptr;
        EXPECT(says(q.make_sizes(d.a), "has bytes but no values"));
    }
}

// The pieces of a copy are windows on the destination's 16-byte grid.
static void pieces() {
    alignas(16) static uint8_t room[4 * concat::kConcatPiece];
    const uint32_t P = concat::kConcatPiece;
    auto n = [&](uint32_t dst_at, uint64_t bytes) { return concat::span_pieces({nullptr, room + dst_at, bytes, 0, 0, 0, 0, 0}); };
    EXPECT(n(0, 0) == 0 && n(5, 0) == 0);
    EXPECT(n(0, 1) == 1 && n(0, P) == 1 && n(0, P + 1) == 2);
    EXPECT(n(1, P - 1) == 1 && n(1, P) == 2 && n(15, P - 15) == 1 && n(15, P - 14) == 2);
    EXPECT(n(17, P - 1) == 1 && n(17, P) == 2);  // the grid starts at the block that holds dst: 16
    EXPECT(n(3, 3ull * P - 3) == 3 && n(3, 3ull * P - 2) == 4);
    auto r = [&](uint64_t offsets) { return concat::span_pieces({nullptr, room, offsets, 0, 0, 0, 8, 0}); };
    EXPECT(r(1) == 1 && r(concat::kConcatOffsetPiece) == 1 && r(concat::kConcatOffsetPiece + 1) == 2);
    std::vector<concat::Span> spans = {{nullptr, room + 1, 2ull * P, 0, 0, 0, 0, 0}, {nullptr, room, 0, 0, 0, 0, 0, 0}, {nullptr, room, 5, 0, 0, 0, 4, 0}};
    std::vector<concat::Item> items;
    concat::add_items(items, spans, 0);
    EXPECT(items.size() == 4 && items[0].span == 0 && items[2].span == 0 && items[2].piece == 2 && items[3].span == 2 && items[3].piece == 0);
}

// The host form stages, of every part and column, only the taken range.
static void staging() {
    Call c;
    c.bits[2] = 5, c.bits[3] = 9;
    const concat::HostStaging in(c.a);
    EXPECT(in.staged.size() == 6);
    const cols::Staging& b = in.block;
    const cols::Staged& i0 = in.staged[0];  // Int32 rows [1, 3) of part 0
    EXPECT(i0.values >= 0 && b.pieces[i0.values].src == c.ints0 + 1 && b.pieces[i0.values].bytes == 8 && i0.validity < 0);
    const cols::Staged& b0 = in.staged[1];  // the boolean: values from bit 5 + 1, validity from bit 9 + 1
    EXPECT(b.pieces[b0.values].src == c.bools0 && b0.vbit == 6 && b.pieces[b0.values].bytes == 1);
    EXPECT(b.pieces[b0.validity].src == c.valid0 + 1 && b0.nbit == 2 && b.pieces[b0.validity].bytes == 1);
    const cols::Staged& t0 = in.staged[2];  // the strings: offsets [1, 3], the span [3, 6)
    EXPECT(b.pieces[t0.offsets].src == c.off0 + 1 && b.pieces[t0.offsets].bytes == 12);
    EXPECT(b.pieces[t0.values].src == (const uint8_t*)c.text0 + 3 && b.pieces[t0.values].bytes == 3 && t0.span_lo == 3);
    for (const cols::Piece& p : b.pieces) EXPECT(p.at % 16 == 0);
    uint8_t block[1];
    EXPECT((uintptr_t)b.values_at(block, t0) + 3 == (uintptr_t)(block + b.pieces[t0.values].at));
    {
        Call d;  // nothing of a part without taken rows
        d.count[0] = 0;
        const concat::HostStaging none(d.a);
        EXPECT(none.staged[0].values < 0 && none.staged[2].offsets < 0 && none.staged[3].values >= 0);
    }
    uint64_t need[3] = {16, 1, 6};
    const concat::OutBlock where(c.a, 4, need);
    EXPECT(where.at == (std::vector<uint64_t>{0, 16, 32, 32, 48, 64, 64, 80, 96}) && where.total == 128);
}

int main() {
    arguments();
    plan();
    pieces();
    staging();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
