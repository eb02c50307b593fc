// tests/native/group_rows_host_test.cpp -- the host-only pieces of oxh_group_rows_* (oxen_amd/csrc/
// group_rows_host.hpp over sort_rows_host.hpp and columns.hpp) in a program of their own: the argument checks
// in the header's order -- the sort's list, then stats4 --, the layout of the leased device memory, and the host
// form's staging plan. No HIP and no library: g++ -std=c++17 (add -fsanitize=address,undefined for a sanitizer
// run). Prints "ok" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstring>

#include "../../oxen_amd/csrc/group_rows_host.hpp"

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

// Three key columns of 3 rows: Int32, Boolean, BYTES32.
struct Call {
    int32_t ints[3] = {1, -2, 3};
    uint8_t bools[1] = {0b101};
    char text[7] = "abcdef";
    int32_t off[4] = {1, 3, 3, 6};
    uint8_t valid[1] = {0b011};
    uint32_t kinds[3] = {OXH_COL_FIXED4, OXH_COL_BOOL, OXH_COL_BYTES32};
    const void* values[3] = {ints, bools, text};
    const void* offsets[3] = {nullptr, nullptr, off};
    const uint8_t* validity[3] = {nullptr, valid, nullptr};
    uint64_t bits[6] = {0, 0, 0, 0, 0, 0};
    uint32_t orders[3] = {OXH_SORT_SIGNED, 0, 0};
    uint32_t group[3] = {9, 9, 9}, count[3] = {9, 9, 9}, first_idx[3] = {9, 9, 9}, first_count[3] = {9, 9, 9};
    uint64_t stats[4] = {7, 7, 7, 7};
    grouprows::Args a{3, 3, kinds, values, offsets, validity, bits, orders, group, count, first_idx, first_count, stats};
};

static void arguments() {
    for (const bool host : {true, false}) {
        Call c;
        EXPECT(grouprows::argument_error(c.a, host).empty());
        { Call d; d.a.kinds = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.values = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.offsets = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.validity = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.bit_offsets = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.orders = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.nkeys = 0; EXPECT(says(grouprows::argument_error(d.a, host), "nkeys is 0")); }
        { Call d; d.kinds[1] = 33; EXPECT(says(grouprows::argument_error(d.a, host), "unknown kind")); }
        { Call d; d.orders[0] = 3; EXPECT(says(grouprows::argument_error(d.a, host), "unknown order class")); }
        { Call d; d.orders[1] = 77, d.orders[2] = 99; EXPECT(grouprows::argument_error(d.a, host).empty()); }  // ignored there
        { Call d; d.kinds[0] = OXH_COL_FIXED1, d.orders[0] = OXH_SORT_FLOAT; EXPECT(says(grouprows::argument_error(d.a, host), "width of 4 or 8")); }
        { Call d; d.orders[0] = OXH_SORT_FLOAT; EXPECT(grouprows::argument_error(d.a, host).empty()); }
        { Call d; d.a.nrows = 0xFFFFFFFFull; EXPECT(says(grouprows::argument_error(d.a, host), "2^32 - 2")); }
        { Call d; d.offsets[2] = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "without offsets")); }
        { Call d; d.values[0] = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "has no values")); }
        { Call d; d.a.stats4 = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "stats4 is NULL")); }
        // every output array may be NULL, alone or together
        for (int mask = 0; mask < 16; ++mask) {
            Call d;
            if (mask & 1) d.a.group = nullptr;
            if (mask & 2) d.a.count = nullptr;
            if (mask & 4) d.a.first_idx = nullptr;
            if (mask & 8) d.a.first_count = nullptr;
            EXPECT(grouprows::argument_error(d.a, host).empty());
        }
        {   // the offsets are read only where they are host memory
            Call d;
            d.off[2] = 2;
            EXPECT(host ? says(grouprows::argument_error(d.a, host), "decrease") : grouprows::argument_error(d.a, host).empty());
            d.off[2] = 3, d.off[0] = -1;
            EXPECT(host ? says(grouprows::argument_error(d.a, host), "negative") : grouprows::argument_error(d.a, host).empty());
            d.off[0] = 1, d.values[2] = nullptr;
            EXPECT(host ? says(grouprows::argument_error(d.a, host), "bytes but no values") : grouprows::argument_error(d.a, host).empty());
            d.off[0] = d.off[1] = d.off[2] = d.off[3] = 4;  // an empty span needs no values
            EXPECT(grouprows::argument_error(d.a, host).empty());
        }
        // the order of the checks
        { Call d; d.a.kinds = nullptr, d.a.nkeys = 0; EXPECT(says(grouprows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.nkeys = 0, d.kinds[0] = 33; EXPECT(says(grouprows::argument_error(d.a, host), "nkeys is 0")); }
        { Call d; d.kinds[1] = 33, d.a.nrows = 1ull << 33; EXPECT(says(grouprows::argument_error(d.a, host), "unknown kind")); }
        { Call d; d.kinds[0] = 1, d.orders[0] = 2, d.a.nrows = 1ull << 33; EXPECT(says(grouprows::argument_error(d.a, host), "width of 4 or 8")); }
        { Call d; d.a.nrows = 1ull << 33, d.a.stats4 = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "2^32 - 2")); }
        { Call d; d.offsets[2] = nullptr, d.a.stats4 = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "without offsets")); }
        // no rows: the arrays of the columns are not looked at, stats4 still is
        { Call d; d.a.nrows = 0, d.values[0] = nullptr, d.offsets[2] = nullptr; EXPECT(grouprows::argument_error(d.a, host).empty()); }
        { Call d; d.a.nrows = 0, d.a.stats4 = nullptr; EXPECT(says(grouprows::argument_error(d.a, host), "stats4 is NULL")); }
        { Call d; d.a.nrows = 0, d.a.nkeys = 0; EXPECT(says(grouprows::argument_error(d.a, host), "nkeys is 0")); }
        EXPECT(c.group[0] == 9 && c.count[1] == 9 && c.first_idx[2] == 9 && c.first_count[0] == 9 && c.stats[3] == 7);
    }
}

static void lease() {
    for (const uint64_t n : {1ull, 63ull, 2048ull, 2049ull, 524291ull, 0xFFFFFFFEull}) {
        const grouprows::Lease at(n);
        // 256-B aligned pieces that do not overlap, in this order, 40 B per row and the scan's sums
        EXPECT(at.digests == 0 && at.first >= at.digests + n * 16 && at.count_of >= at.first + n * 8);
        EXPECT(at.flag >= at.count_of + n * 4 && at.flag_scan >= at.flag + n * 4 && at.sums >= at.flag_scan + n * 8);
        EXPECT(at.total >= at.sums + (grouprows::scan_tiles_of(n) + 1) * 8);
        for (const uint64_t x : {at.first, at.count_of, at.flag, at.flag_scan, at.sums, at.total}) EXPECT(x % 256 == 0);
        EXPECT(at.total <= n * 40 + 6 * 256 + (n / 2048 + 2) * 8);
    }
    EXPECT(grouprows::scan_tiles_of(0) == 0 && grouprows::scan_tiles_of(1) == 1 && grouprows::scan_tiles_of(2048) == 1 &&
           grouprows::scan_tiles_of(2049) == 2);
    EXPECT(grouprows::kMaxRows == 0xFFFFFFFEull);
}

static void plan() {
    Call c;
    c.bits[2] = 0, c.bits[3] = 13;   // the boolean's validity starts at bit 13
    uint8_t wide_valid[3] = {0, 0b01100000, 0};
    c.validity[1] = wide_valid;
    const grouprows::HostPlan p(c.a);
    EXPECT(p.out_bytes == 16);              // 3 u32, 16-B aligned
    EXPECT(p.staging.pieces.size() == 5);   // ints; bools + validity; offsets + span
    EXPECT(p.staging.pieces[0].at == 64 && p.staging.pieces[0].bytes == 12);  // behind the four output arrays
    EXPECT(p.staged[1].nbit == 5 && p.staging.pieces[p.staged[1].validity].src == wide_valid + 1 && p.staging.pieces[p.staged[1].validity].bytes == 1);
    EXPECT(p.staged[2].span_lo == 1 && p.staging.pieces[p.staged[2].values].bytes == 5 && p.staging.pieces[p.staged[2].offsets].bytes == 16);
    uint8_t* block = (uint8_t*)0x10000;
    EXPECT(p.staging.values_at(block, p.staged[2]) == block + p.staging.pieces[p.staged[2].values].at - 1);
    EXPECT(p.staging.total % 16 == 0 && p.staging.total >= 64 + 5 * 16);
}

int main() {
    arguments();
    lease();
    plan();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
