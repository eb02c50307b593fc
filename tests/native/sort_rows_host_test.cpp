// tests/native/sort_rows_host_test.cpp -- the host-only pieces of oxh_sort_rows_* (oxen_amd/csrc/
// sort_rows_host.hpp, sort_keys.hpp, columns.hpp) in a program of their own: the argument checks in the
// header's order, the host form's staging plan, and the key words the kernels build -- for every order class
// `encode(a) < encode(b)` against the comparator the header states, and class, word and tail of the string
// cases. No HIP and no library: g++ -std=c++17 (add -fsanitize=address,undefined for a sanitizer run). Prints
// "ok" and exits 0, or says what failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../oxen_amd/csrc/sort_rows_host.hpp"

using namespace oxh;
namespace sk = oxh::sortkeys;

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
    uint32_t perm[3] = {9, 9, 9};
    uint64_t stats[3] = {7, 7, 7};
    sortrows::Args a{3, 3, kinds, values, offsets, validity, bits, orders, perm, stats};
};

static void arguments() {
    for (const bool host : {true, false}) {
        Call c;
        EXPECT(sortrows::argument_error(c.a, host).empty());
        // each NULL table array
        { Call d; d.a.kinds = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.values = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.offsets = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.validity = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.bit_offsets = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.orders = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.nkeys = 0; EXPECT(says(sortrows::argument_error(d.a, host), "nkeys is 0")); }
        { Call d; d.kinds[1] = 33; EXPECT(says(sortrows::argument_error(d.a, host), "unknown kind")); }
        { Call d; d.orders[0] = 3; EXPECT(says(sortrows::argument_error(d.a, host), "unknown order class")); }
        { Call d; d.orders[1] = 77, d.orders[2] = 99; EXPECT(sortrows::argument_error(d.a, host).empty()); }  // ignored there
        { Call d; d.kinds[0] = OXH_COL_FIXED1, d.orders[0] = OXH_SORT_FLOAT; EXPECT(says(sortrows::argument_error(d.a, host), "width of 4 or 8")); }
        { Call d; d.orders[0] = OXH_SORT_FLOAT; EXPECT(sortrows::argument_error(d.a, host).empty()); }
        { Call d; d.a.nrows = 0xFFFFFFFFull; EXPECT(says(sortrows::argument_error(d.a, host), "2^32 - 2")); }
        { Call d; d.offsets[2] = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "without offsets")); }
        { Call d; d.values[0] = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "has no values")); }
        { Call d; d.a.perm = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "perm is NULL")); }
        { Call d; d.a.stats3 = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "stats3 is NULL")); }
        {   // the offsets are read only where they are host memory
            Call d;
            d.off[2] = 2;
            EXPECT(host ? says(sortrows::argument_error(d.a, host), "decrease") : sortrows::argument_error(d.a, host).empty());
            d.off[2] = 3, d.off[0] = -1;
            EXPECT(host ? says(sortrows::argument_error(d.a, host), "negative") : sortrows::argument_error(d.a, host).empty());
            d.off[0] = 1, d.values[2] = nullptr;
            EXPECT(host ? says(sortrows::argument_error(d.a, host), "bytes but no values") : sortrows::argument_error(d.a, host).empty());
            d.off[0] = d.off[1] = d.off[2] = d.off[3] = 4;  // an empty span needs no values
            EXPECT(sortrows::argument_error(d.a, host).empty());
        }
        // the order of the checks
        { Call d; d.a.kinds = nullptr, d.a.nkeys = 0; EXPECT(says(sortrows::argument_error(d.a, host), "is NULL")); }
        { Call d; d.a.nkeys = 0, d.kinds[0] = 33; EXPECT(says(sortrows::argument_error(d.a, host), "nkeys is 0")); }
        { Call d; d.kinds[1] = 33, d.a.nrows = 1ull << 33; EXPECT(says(sortrows::argument_error(d.a, host), "unknown kind")); }
        { Call d; d.kinds[0] = 1, d.orders[0] = 2, d.a.nrows = 1ull << 33; EXPECT(says(sortrows::argument_error(d.a, host), "width of 4 or 8")); }
        { Call d; d.a.nrows = 1ull << 33, d.a.perm = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "2^32 - 2")); }
        { Call d; d.offsets[2] = nullptr, d.a.perm = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "without offsets")); }
        { Call d; d.a.perm = nullptr, d.a.stats3 = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "perm is NULL")); }
        // no rows: the arrays of the columns and perm are not looked at, stats3 still is
        { Call d; d.a.nrows = 0, d.values[0] = nullptr, d.offsets[2] = nullptr, d.a.perm = nullptr; EXPECT(sortrows::argument_error(d.a, host).empty()); }
        { Call d; d.a.nrows = 0, d.a.stats3 = nullptr; EXPECT(says(sortrows::argument_error(d.a, host), "stats3 is NULL")); }
        { Call d; d.a.nrows = 0, d.a.nkeys = 0; EXPECT(says(sortrows::argument_error(d.a, host), "nkeys is 0")); }
        EXPECT(c.perm[0] == 9 && c.stats[0] == 7);
    }
}

static void plan() {
    Call c;
    c.bits[2] = 0, c.bits[3] = 13;   // the boolean's validity starts at bit 13
    uint8_t wide_valid[3] = {0, 0b01100000, 0};
    c.validity[1] = wide_valid;
    const sortrows::HostPlan p(c.a);
    EXPECT(p.staging.pieces.size() == 5);  // ints; bools + validity; offsets + span
    EXPECT(p.staging.pieces[0].at == 16 && p.staging.pieces[0].bytes == 12);  // behind the 3 u32 of perm, 16-B aligned
    EXPECT(p.staged[1].nbit == 5 && p.staging.pieces[p.staged[1].validity].src == wide_valid + 1 && p.staging.pieces[p.staged[1].validity].bytes == 1);
    EXPECT(p.staged[2].span_lo == 1 && p.staging.pieces[p.staged[2].values].bytes == 5 && p.staging.pieces[p.staged[2].offsets].bytes == 16);
    uint8_t* block = (uint8_t*)0x10000;
    EXPECT(p.staging.values_at(block, p.staged[2]) == block + p.staging.pieces[p.staged[2].values].at - 1);
    EXPECT(p.staging.total % 16 == 0 && p.staging.total >= 16 + 16 + 16 + 16 + 16 + 16);
}

// ---------------------------------------------------------------- the key words against the stated order
template <class T>
static uint64_t raw_of(T v) {
    uint64_t r = 0;
    std::memcpy(&r, &v, sizeof v);
    return r;
}

template <class T>
static void integers(uint32_t order) {
    const T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
    const T vals[] = {lo, (T)(lo + 1), (T)-1, 0, 1, 2, (T)(hi / 2), (T)(hi / 2 + 1), (T)(hi - 1), hi, (T)0x80, (T)0x7F};
    for (T a : vals)
        for (T b : vals) {
            const uint64_t ea = sk::fixed_word(order, sizeof(T), raw_of(a)), eb = sk::fixed_word(order, sizeof(T), raw_of(b));
            EXPECT((ea < eb) == (a < b));
            EXPECT((ea == eb) == (a == b));
        }
}

template <class F, class U>
static F from_bits(U bits) {
    F f;
    std::memcpy(&f, &bits, sizeof f);
    return f;
}

// the header's float order: numeric, -0.0 == +0.0, every NaN equal to every NaN and above +inf
template <class F>
static bool float_less(F a, F b) {
    if (std::isnan(a)) return false;
    if (std::isnan(b)) return true;
    return a < b;
}

template <class F, class U>
static void floats(const U* nan_bits, int nnans) {
    std::vector<F> vals = {(F)0.0, (F)-0.0, (F)1.0, (F)-1.0, std::numeric_limits<F>::infinity(), -std::numeric_limits<F>::infinity(),
                           std::numeric_limits<F>::denorm_min(), -std::numeric_limits<F>::denorm_min(), std::numeric_limits<F>::min(),
                           -std::numeric_limits<F>::min(), std::numeric_limits<F>::max(), std::numeric_limits<F>::lowest(), (F)1.5,
                           (F)-1.5, (F)3e-40, (F)-3e-40};
    for (int k = 0; k < nnans; ++k) vals.push_back(from_bits<F, U>(nan_bits[k]));
    for (F a : vals)
        for (F b : vals) {
            const uint64_t ea = sk::fixed_word(OXH_SORT_FLOAT, sizeof(F), raw_of(a)), eb = sk::fixed_word(OXH_SORT_FLOAT, sizeof(F), raw_of(b));
            EXPECT((ea < eb) == float_less(a, b));
            EXPECT((ea == eb) == (!float_less(a, b) && !float_less(b, a)));
        }
}

static void fixed_words() {
    integers<int8_t>(OXH_SORT_SIGNED);
    integers<int32_t>(OXH_SORT_SIGNED);
    integers<int64_t>(OXH_SORT_SIGNED);
    integers<uint8_t>(OXH_SORT_UNSIGNED);
    integers<uint32_t>(OXH_SORT_UNSIGNED);
    integers<uint64_t>(OXH_SORT_UNSIGNED);
    const uint32_t nan32[] = {0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFF800001u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0x7FA55AA5u};
    const uint64_t nan64[] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, 0xFFF0000000000001ull,
                              0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull, 0x7FF5A5A5A5A5A5A5ull};
    floats<float, uint32_t>(nan32, 7);
    floats<double, uint64_t>(nan64, 7);
    // a present cell of any class is class "present" with tail 0; a null is below it whatever the word
    const sk::Triple t = sk::fixed_triple(OXH_SORT_SIGNED, 8, raw_of(std::numeric_limits<int64_t>::min()));
    EXPECT(t.cls == sk::kClassPresent && t.tail == 0 && t.word == 0);
    EXPECT(sk::less(sk::null_triple(), t) && !sk::less(t, sk::null_triple()));
    EXPECT(sk::less(sk::bool_triple(false), sk::bool_triple(true)) && sk::less(sk::null_triple(), sk::bool_triple(false)));
    EXPECT(!sk::next_chunk(t) && !sk::next_chunk(sk::null_triple()));
}

// memcmp order with a proper prefix first
static bool bytes_less(const std::string& a, const std::string& b) {
    const size_t n = std::min(a.size(), b.size());
    const int c = std::memcmp(a.data(), b.data(), n);
    return c ? c < 0 : a.size() < b.size();
}

// the order the rounds give two present byte cells: chunk by chunk until the triples differ or the cells end
static int rounds_compare(const std::string& a, const std::string& b, int* rounds) {
    for (uint64_t chunk = 0;; ++chunk) {
        // an exact-size copy of each cell: a sanitizer build sees any read past the cell
        std::vector<uint8_t> ca(a.begin(), a.end()), cb(b.begin(), b.end());
        const sk::Triple ta = sk::bytes_triple(ca.data(), ca.size(), chunk), tb = sk::bytes_triple(cb.data(), cb.size(), chunk);
        *rounds = (int)chunk + 1;
        if (sk::less(ta, tb)) return -1;
        if (sk::less(tb, ta)) return 1;
        if (!sk::next_chunk(ta)) return 0;
    }
}

static void byte_words() {
    using S = std::string;
    // the ladder of the header: "" < "a" < "a\0" < "a\0\0" < "b", a null before ""
    const S ladder[] = {S(""), S("a"), S("a\0", 2), S("a\0\0", 3), S("b")};
    {
        const sk::Triple e = sk::bytes_triple(nullptr, 0, 0), a = sk::bytes_triple((const uint8_t*)"a", 1, 0);
        EXPECT(e.cls == sk::kClassExhausted && e.tail == 0 && e.word == 0 && sk::less(sk::null_triple(), e));
        EXPECT(a.cls == sk::kClassPresent && a.tail == 1 && a.word == 0x6100000000000000ull);
        const sk::Triple a0 = sk::bytes_triple((const uint8_t*)"a\0", 2, 0), a00 = sk::bytes_triple((const uint8_t*)"a\0\0", 3, 0);
        EXPECT(a0.word == a.word && a0.tail == 2 && a00.word == a.word && a00.tail == 3);
        const sk::Triple full = sk::bytes_triple((const uint8_t*)"abcdefgh", 8, 0), after = sk::bytes_triple((const uint8_t*)"abcdefgh", 8, 1);
        EXPECT(full.tail == 8 && full.word == 0x6162636465666768ull && sk::next_chunk(full) && !sk::next_chunk(a));
        EXPECT(after.cls == sk::kClassExhausted && !sk::next_chunk(after));
        const sk::Triple second = sk::bytes_triple((const uint8_t*)"abcdefghij", 10, 1);
        EXPECT(second.cls == sk::kClassPresent && second.tail == 2 && second.word == 0x696A000000000000ull);
        EXPECT(sk::bytes_triple((const uint8_t*)"ab", 2, ~0ull).cls == sk::kClassExhausted);  // no overflow in 8 * chunk
        const uint8_t high[2] = {0x80, 0xFF};
        EXPECT(sk::less(sk::bytes_triple((const uint8_t*)"\x7F", 1, 0), sk::bytes_triple(high, 2, 0)));  // unsigned bytes
    }
    std::vector<S> cells(ladder, ladder + 5);
    for (const char* s : {"abcdefg", "abcdefgh", "abcdefghi", "abcdefgh\0", "abcdefgz", "abcdefghabcdefgh", "abcdefghabcdefg", "\x80", "\xFF\xFF"})
        cells.push_back(s == S("abcdefgh\0") ? S("abcdefgh\0", 9) : S(s));
    cells.push_back(S(64, 'p') + "a");
    cells.push_back(S(64, 'p') + "b");
    cells.push_back(S(64, 'p'));
    for (const S& a : cells)
        for (const S& b : cells) {
            int rounds = 0;
            const int c = rounds_compare(a, b, &rounds);
            EXPECT((c < 0) == bytes_less(a, b) && (c > 0) == bytes_less(b, a));
            if (a.size() == 65 && b.size() == 65 && a != b) EXPECT(rounds == 9);  // the ninth chunk holds byte 64
        }
    // the second key word: stable passes over byte 0, the word, bytes 1.. order by (group, class, word, tail)
    const sk::Triple t{sk::kClassPresent, 8, 5};
    const uint64_t m = sk::pack_meta(0xFFFFFFFEu, t);
    EXPECT(sk::meta_tail(m) == 8 && sk::meta_class(m) == sk::kClassPresent && m >> 16 == 0xFFFFFFFEull);
}

int main() {
    arguments();
    plan();
    fixed_words();
    byte_words();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
