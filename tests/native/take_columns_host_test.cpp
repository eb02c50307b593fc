// tests/native/take_columns_host_test.cpp -- the host-only pieces of oxh_take_columns_* (oxen_amd/csrc/
// take_columns_host.hpp, columns.hpp) in a program of their own: the argument checks in the header's order,
// the host forms' staging plan of a column (only what the rows name, the residual bit offsets, the rebased
// values pointer) and the layout of the host form's output block. No HIP and no library: g++ -std=c++17
// (add -fsanitize=address,undefined for a sanitizer run). Prints "ok" and exits 0, or says what failed and
// exits 1.
#include <cstdio>
#include <cstring>

#include "../../oxen_amd/csrc/take_columns_host.hpp"

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

// Three source columns -- Int32 of 3 rows, Boolean of 3 rows, BYTES32 of 2 rows -- and three output columns of
// 4 rows: a plain take of each, the first with itself as the fallback through the other index array.
struct Call {
    int32_t ints[3] = {1, 2, 3};
    uint8_t bools[1] = {0b101};
    char text[7] = "abcdef";
    int32_t off[3] = {1, 3, 6};
    uint8_t valid[1] = {0b011};
    uint32_t kinds[3] = {OXH_COL_FIXED4, OXH_COL_BOOL, OXH_COL_BYTES32};
    const void* values[3] = {ints, bools, text};
    const void* offsets[3] = {nullptr, nullptr, off};
    const uint8_t* validity[3] = {nullptr, valid, nullptr};
    uint64_t bits[6] = {0, 0, 0, 0, 0, 0};
    uint64_t rows[3] = {3, 3, 2};
    uint32_t idx0[4] = {0, 2, OXH_TAKE_NULL, 1}, idx1[4] = {1, OXH_TAKE_NULL, 0, 0};
    uint32_t plan[12] = {0, 0, 0, 1, 1, 0, OXH_TAKE_NO_COLUMN, 0, 2, 1, OXH_TAKE_NO_COLUMN, 0};
    uint64_t capacity[3] = {0, 0, 64};
    alignas(8) uint8_t v0[16], v1[8], v2[64], n0[8], n1[8], n2[8];
    int32_t o2[5];
    void* out_values[3] = {v0, v1, v2};
    void* out_offsets[3] = {nullptr, nullptr, o2};
    uint8_t* out_validity[3] = {n0, n1, n2};
    uint64_t value_bytes[3] = {7, 7, 7};
    uint32_t written = 7;
    take::Args a{3, kinds, values, offsets, validity, bits, rows, 4, idx0, idx1, 3, plan, capacity, out_values, out_offsets,
                 out_validity, value_bytes, &written};
};

static void arguments() {
    for (const bool host : {true, false}) {
        Call c;
        EXPECT(take::argument_error(c.a, host).empty());
        {
            Call d;  // the sizes-only call: value_capacity is not looked at
            d.a.out_values = nullptr, d.a.out_offsets = nullptr, d.a.out_validity = nullptr, d.a.value_capacity = nullptr;
            EXPECT(take::argument_error(d.a, host).empty() && take::sizes_only(d.a));
        }
#define BAD(change, part)                                   \
    do {                                                    \
        Call d;                                             \
        change;                                             \
        EXPECT(says(take::argument_error(d.a, host), part)); \
    } while (0)
        BAD(d.a.kinds = nullptr, "is NULL");
        BAD(d.a.values = nullptr, "is NULL");
        BAD(d.a.offsets = nullptr, "is NULL");
        BAD(d.a.validity = nullptr, "is NULL");
        BAD(d.a.bit_offsets = nullptr, "is NULL");
        BAD(d.a.src_rows = nullptr, "is NULL");
        BAD(d.a.plan = nullptr, "is NULL");
        BAD(d.a.nsrc = 0, "nsrc or nout is 0");
        BAD(d.a.nout = 0, "nsrc or nout is 0");
        BAD(d.kinds[1] = 33, "unknown kind");
        BAD(d.plan[4] = 3, "not there");
        BAD(d.plan[2] = 3, "not there");
        BAD(d.plan[5] = 2, "index array");
        BAD(d.plan[3] = 2, "index array");
        BAD(d.plan[6] = 0, "kind differs");          // Boolean with an Int32 fallback
        BAD(d.a.nout_rows = 0xFFFFFFFFull, "2^32 - 2 output rows");
        BAD(d.rows[1] = 0xFFFFFFFFull, "2^32 - 2 rows");
        BAD(d.a.value_bytes = nullptr, "value_bytes or written");
        BAD(d.a.written = nullptr, "value_bytes or written");
        BAD(d.offsets[2] = nullptr, "without offsets");
        BAD(d.values[0] = nullptr, "has no values");
        BAD(d.a.out_values = nullptr, "some of");
        BAD(d.a.out_validity = nullptr, "some of");
        BAD(d.a.value_capacity = nullptr, "value_capacity");
        BAD(d.out_offsets[2] = nullptr, "without out_offsets");
        BAD(d.out_validity[1] = nullptr, "no out_validity");
        BAD(d.out_values[0] = nullptr, "no out_values");
        BAD(d.out_values[2] = nullptr, "no out_values");   // a byte column with capacity
        if (host) {
            BAD(d.off[1] = 0, "decrease");
            BAD(d.off[0] = -1, "negative");
            BAD(d.values[2] = nullptr, "bytes but no values");
            Call d;  // the host form's outputs need no alignment
            d.out_validity[0] = d.n0 + 1, d.out_values[1] = d.v1 + 3;
            EXPECT(take::argument_error(d.a, true).empty());
        } else {
            BAD(d.out_validity[0] = d.n0 + 4, "8-byte aligned");
            BAD(d.out_values[1] = d.v1 + 1, "8-byte aligned");
            Call d;  // what is not bit-packed may sit anywhere; the offsets are on the device and not read
            d.out_values[0] = d.v0 + 1, d.off[1] = 0;
            EXPECT(take::argument_error(d.a, false).empty());
        }
        // the order of the header
        BAD((d.a.kinds = nullptr, d.a.nsrc = 0, d.kinds[0] = 9), "is NULL");
        BAD((d.a.nsrc = 0, d.kinds[0] = 9), "nsrc or nout");
        BAD((d.kinds[0] = 9, d.plan[0] = 7), "unknown kind");
        BAD((d.plan[0] = 7, d.plan[6] = 0), "not there");
        BAD((d.plan[6] = 0, d.a.nout_rows = 1ull << 33), "kind differs");
        BAD((d.a.nout_rows = 1ull << 33, d.a.written = nullptr), "2^32 - 2");
        BAD((d.a.written = nullptr, d.offsets[2] = nullptr), "value_bytes or written");
        BAD((d.offsets[2] = nullptr, d.values[0] = nullptr), "without offsets");
        BAD((d.values[0] = nullptr, d.a.out_values = nullptr), "has no values");
#undef BAD
        // a column without rows: its arrays are not looked at; no output rows: only the byte columns' offsets are
        Call e;
        e.rows[2] = 0, e.offsets[2] = nullptr, e.values[2] = nullptr;
        EXPECT(take::argument_error(e.a, host).empty());
        Call z;
        z.a.nout_rows = 0, z.out_validity[0] = nullptr, z.out_values[1] = nullptr;
        EXPECT(take::argument_error(z.a, host).empty());
        z.out_offsets[2] = nullptr;
        EXPECT(says(take::argument_error(z.a, host), "without out_offsets"));
    }
}

static void staging() {
    // a byte column of 3 rows sliced out of a longer one: offsets[0] = 5, validity from bit 13
    const char bytes[] = "0123456789abcdefghij";
    const int32_t off[4] = {5, 5, 9, 17};
    const uint8_t valid[4] = {0xFF, 0xFF, 0xFF, 0xFF};
    cols::Staging plan;
    plan.total = 32;  // a caller's own front
    const cols::Staged s = plan.add_column(OXH_COL_BYTES32, bytes, off, valid, 0, 13, 3);
    EXPECT(s.span_lo == 5 && s.nbit == 5 && s.vbit == 0 && s.offsets >= 0 && s.values >= 0 && s.validity >= 0);
    EXPECT(plan.pieces.size() == 3 && plan.total % 16 == 0);
    const cols::Piece &po = plan.pieces[s.offsets], &pv = plan.pieces[s.values], &pn = plan.pieces[s.validity];
    EXPECT(po.src == off && po.bytes == 16 && po.at == 32);
    EXPECT(pv.src == bytes + 5 && pv.bytes == 12 && pv.at == 48);           // exactly [offsets[0], offsets[3])
    EXPECT(pn.src == valid + 1 && pn.bytes == 1 && pn.at == 64);            // bits 13 .. 15: one byte, residual offset 5
    // the block as a host buffer: what the pieces say, then the cells through the rebased pointer
    std::vector<uint8_t> block(plan.total, 0xEE);
    for (const cols::Piece& p : plan.pieces) std::memcpy(block.data() + p.at, p.src, p.bytes);
    const uint8_t* values = (const uint8_t*)plan.values_at(block.data(), s);
    const int32_t* offsets = (const int32_t*)plan.offsets_at(block.data(), s);
    EXPECT(plan.validity_at(block.data(), s) == block.data() + 64);
    for (int r = 0; r < 3; ++r)
        EXPECT(!std::memcmp(values + offsets[r], bytes + off[r], (size_t)(off[r + 1] - off[r])));
    // a boolean column from bit 3 over 14 rows, validity from bit 0; an empty span has no values piece
    const uint8_t bools[3] = {0xAA, 0x55, 0xAA};
    const cols::Staged b = plan.add_column(OXH_COL_BOOL, bools, nullptr, valid, 3, 0, 14);
    EXPECT(b.vbit == 3 && b.nbit == 0 && plan.pieces[b.values].bytes == 3 && plan.pieces[b.validity].bytes == 2 && b.offsets < 0);
    const int32_t none[3] = {4, 4, 4};
    const cols::Staged e = plan.add_column(OXH_COL_BYTES32, nullptr, none, nullptr, 0, 0, 2);
    EXPECT(e.values < 0 && e.validity < 0 && plan.values_at(block.data(), e) == nullptr && plan.validity_at(block.data(), e) == nullptr);
    const int64_t wide[3] = {0, 2, 5};
    const cols::Staged w = plan.add_column(OXH_COL_BYTES64, bytes, wide, nullptr, 0, 0, 2);
    EXPECT(plan.pieces[w.offsets].bytes == 24 && plan.pieces[w.values].bytes == 5);
    const double f[4] = {1, 2, 3, 4};
    EXPECT(plan.pieces[plan.add_column(OXH_COL_FIXED8, f, nullptr, nullptr, 0, 0, 4).values].bytes == 32);
    // the kinds
    EXPECT(cols::width_of(OXH_COL_FIXED1) == 1 && cols::width_of(OXH_COL_FIXED8) == 8 && cols::width_of(OXH_COL_BOOL) == 0);
    EXPECT(cols::offset_width(OXH_COL_BYTES32) == 4 && cols::offset_width(OXH_COL_BYTES64) == 8);
    EXPECT(cols::known_kind(OXH_COL_BYTES64) && !cols::known_kind(0) && !cols::known_kind(2));
}

static void output_block() {
    Call c;
    c.a.nout_rows = 70;
    const uint64_t need[3] = {280, 9, 1001};
    const take::OutBlock where(c.a, need);
    EXPECT(take::plain_value_bytes(OXH_COL_FIXED4, 70) == 280 && take::plain_value_bytes(OXH_COL_BOOL, 70) == 9);
    uint64_t end = 0;
    for (uint32_t o = 0; o < 3; ++o) {
        const uint64_t sizes[3] = {take::bitmap_bytes(70), need[o], o == 2 ? 71 * 4ull : 0};
        for (int k = 0; k < 3; ++k) {
            EXPECT(where.at[3 * o + k] % 16 == 0 && where.at[3 * o + k] >= end);  // aligned, in order, no overlap
            end = where.at[3 * o + k] + sizes[k];
        }
    }
    EXPECT(where.total >= end && where.total % 16 == 0);
}

int main() {
    arguments();
    staging();
    output_block();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
