// tests/native/csv_write_host_test.cpp -- the CSV writer's text functions on the CPU (oxen_amd/csrc/csv_text.hpp,
// the code the kernels of csv_write.hip compile): the integer text at its edges, the float text over a table of edge
// values, the quoting, and the exact path against std::to_chars over 10 M and more values of four classes with a
// fixed seed -- zero mismatches among the values it accepts; the hit rate is printed and is no threshold.
// Build: g++ -std=c++17 -O2 -Wall -o csv_write_host_test csv_write_host_test.cpp   (oxen_amd/build.py does)
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../oxen_amd/csrc/csv_text.hpp"

namespace t = oxh::csvtext;

static const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
static int g_failures = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++g_failures;                     \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);     \
            fputc('\n', stderr);              \
        }                                     \
    } while (0)

static uint64_t bits_of(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

static double double_of(uint64_t b) {
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// The writer's text of one double, as a call produces it: the device's own text, or the host's slot.
static std::string float_text(uint64_t bits, bool* deferred = nullptr) {
    uint8_t buf[t::kDeferSlot + 8];
    memset(buf, '#', sizeof buf);
    const t::FloatForm f = t::float_form(bits, kPow10);
    if (deferred) *deferred = f.kind == t::kFormDeferred;
    if (f.kind == t::kFormDeferred) {
        t::deferred_slot(bits, buf);
        const uint32_t n = buf[t::kDeferSlot - 1];
        CHECK(n <= t::kMaxFloatText, "a slot of %u bytes", n);
        return std::string((const char*)buf, n);
    }
    const uint32_t n = t::form_text(f, nullptr);
    CHECK(n <= t::kMaxFloatText, "a text of %u bytes", n);
    CHECK(t::form_text(f, buf) == n, "the measured and the written length differ");
    CHECK(buf[n] == '#', "a byte behind the text was written");
    return std::string((const char*)buf, n);
}

static std::string int_text(int64_t v) {
    uint8_t buf[24];
    memset(buf, '#', sizeof buf);
    const uint32_t n = t::int64_text(v, nullptr);
    CHECK(t::int64_text(v, buf) == n && buf[n] == '#', "int64_text(%lld): measured and written differ", (long long)v);
    return std::string((const char*)buf, n);
}

static void test_integers() {
    CHECK(int_text(0) == "0", "0");
    CHECK(int_text(1) == "1", "1");
    CHECK(int_text(-1) == "-1", "-1");
    CHECK(int_text(INT64_MAX) == "9223372036854775807", "max");
    CHECK(int_text(INT64_MIN) == "-9223372036854775808", "min");
    int64_t p = 1;
    for (int k = 1; k <= 18; ++k) {
        p *= 10;
        for (int64_t v : {p - 1, p, p + 1, -(p - 1), -p, -(p + 1)}) {
            CHECK(int_text(v) == std::to_string(v), "10^%d neighbourhood: %lld gives %s", k, (long long)v, int_text(v).c_str());
        }
    }
    for (uint64_t v : {0ull, 9ull, 10ull, 9999999999999999999ull, 10000000000000000000ull, 18446744073709551615ull})
        CHECK(t::digits_u64(v) == std::to_string(v).size(), "digits_u64(%llu)", (unsigned long long)v);
}

struct Edge {
    uint64_t bits;
    const char* text;
    int deferred;  // 1 / 0; -1: not stated
};

static void test_float_table() {
    const Edge table[] = {
        {bits_of(0.0), "0.0", 0},
        {bits_of(-0.0), "-0.0", 0},
        {0x7FF8000000000000ull, "NaN", 0},
        {0xFFF8000000000000ull, "NaN", 0},
        {0x7FF0000000000001ull, "NaN", 0},
        {0xFFF80000DEADBEEFull, "NaN", 0},
        {0x7FF0000000000000ull, "inf", 0},
        {0xFFF0000000000000ull, "-inf", 0},
        {bits_of(0.1), "0.1", 0},
        {bits_of(19.0), "19.0", 0},
        {bits_of(-19.0), "-19.0", 0},
        {bits_of(12.5), "12.5", 0},
        {bits_of(1e-5), "0.00001", 0},
        {bits_of(1e-6), "1e-6", 0},
        {bits_of(1.5e-7), "1.5e-7", 0},
        {bits_of(1.25e-7), "1.25e-7", 0},
        {bits_of(-1.25e-7), "-1.25e-7", 0},
        {bits_of(1e-22), "1e-22", 0},
        {bits_of(1e-23), "1e-23", 1},
        {bits_of(999999999999999.0), "999999999999999.0", 0},
        {bits_of(1e14), "100000000000000.0", 0},
        {bits_of(1e15), "1000000000000000.0", 1},
        {bits_of(1e16), "1e16", 1},
        {bits_of(1.5e16), "1.5e16", 1},
        {bits_of(123456789012345680.0), "1.2345678901234568e17", 1},  // 17 digits and kk = 18: the exponent form
        {bits_of(1234567890123456.0), "1234567890123456.0", 1},
        {bits_of(0.1 + 0.2), "0.30000000000000004", 1},
        {bits_of(5e-324), "5e-324", 1},
        {bits_of(2.2250738585072014e-308), "2.2250738585072014e-308", 1},
        {bits_of(-2.2250738585072014e-308), "-2.2250738585072014e-308", 1},
        {bits_of(1.7976931348623157e308), "1.7976931348623157e308", 1},
        {bits_of(0.001), "0.001", 0},
        {bits_of(123.456), "123.456", 0},
        {bits_of(1e21), "1e21", 1},
    };
    for (const Edge& e : table) {
        bool deferred = false;
        const std::string got = float_text(e.bits, &deferred);
        CHECK(got == e.text, "0x%016llx: %s, expected %s", (unsigned long long)e.bits, got.c_str(), e.text);
        if (e.deferred >= 0) CHECK((int)deferred == e.deferred, "%s: deferred %d, expected %d", e.text, (int)deferred, e.deferred);
    }
}

static void test_strings() {
    struct Case {
        const char* in;
        const char* out;
    };
    const Case cases[] = {{"", "\"\""},          {"a", "a"},         {",", "\",\""},         {"\"", "\"\"\"\""},
                          {"\n", "\"\n\""},      {"\r", "\"\r\""},   {"a\"b", "\"a\"\"b\""}, {"\"\"", "\"\"\"\"\"\""},
                          {"a b", "a b"},        {"a\tb", "a\tb"},   {"x,y\"z", "\"x,y\"\"z\""}};
    for (const Case& c : cases) {
        const uint64_t n = strlen(c.in);
        bool quoted = false;
        const uint64_t len = t::string_text_len((const uint8_t*)c.in, n, ',', '"', quoted);
        std::string got;
        if (quoted) {
            std::vector<uint8_t> buf(len + 1, '#');
            t::quoted_text_put((const uint8_t*)c.in, n, '"', buf.data());
            CHECK(buf[len] == '#', "a byte behind the cell was written");
            got.assign((const char*)buf.data(), len);
        } else {
            got.assign(c.in, n);
        }
        CHECK(len == strlen(c.out) && got == c.out, "cell <%s>: <%s>, expected <%s>", c.in, got.c_str(), c.out);
    }
    bool quoted = false;
    CHECK(t::string_text_len((const uint8_t*)"a\tb", 3, '\t', '"', quoted) == 5 && quoted, "the TSV separator is a hazard");
    for (uint32_t c = 0; c < 256; ++c) {
        const bool expected = (c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
        CHECK(t::in_number_text(c) == expected, "in_number_text(%u)", c);
    }
}

static uint64_t g_state = 0x6F78656E2D637376ull;  // the fixed seed
static uint64_t next_u64() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct ClassCount {
    const char* name;
    uint64_t values = 0, hits = 0, mismatches = 0;
};

// One value through the exact path; a hit must give std::to_chars's shortest digits.
static void exact_one(double a, ClassCount& cc) {
    if (!(a > 0) || !(a < INFINITY)) return;
    ++cc.values;
    uint64_t d = 0, hd = 0;
    uint32_t L = 0, hL = 0;
    int32_t k = 0, hk = 0;
    if (!t::exact_digits(a, kPow10, d, L, k)) return;
    ++cc.hits;
    t::shortest_digits_host(a, hd, hL, hk);
    if (d != hd || L != hL || k != hk) {
        if (cc.mismatches++ < 10)
            fprintf(stderr, "MISMATCH %s %.17g: exact %llu e%d, to_chars %llu e%d\n", cc.name, a, (unsigned long long)d, k,
                    (unsigned long long)hd, hk);
    }
}

static void test_exact_path(uint64_t per_class) {
    ClassCount cls[4] = {{"short decimals"}, {"two-decimal prices"}, {"random bit patterns"}, {"dyadic fractions"}};
    for (uint64_t i = 0; i < per_class; ++i) {
        {   // up to 15 digits, a decimal exponent of -25 .. 5: correctly rounded by strtod
            const uint64_t r = next_u64();
            const uint32_t nd = 1 + (uint32_t)(r % 15);
            const uint64_t m = (next_u64() % t::pow10_u64(nd));
            const int e = (int)((r >> 8) % 31) - 25;
            char text[48];
            snprintf(text, sizeof text, "%llue%d", (unsigned long long)m, e);
            exact_one(strtod(text, nullptr), cls[0]);
        }
        {   // prices: cents up to 10^9, as a program computes them
            const uint64_t cents = next_u64() % 1000000000ull;
            exact_one((double)cents / 100.0, cls[1]);
        }
        exact_one(double_of(next_u64() & ~t::kSignBit), cls[2]);
        {   // m / 2^s: exact binary fractions, long decimals
            const uint64_t r = next_u64();
            exact_one(ldexp((double)(r >> 40), -(int)(r % 40)), cls[3]);
        }
    }
    uint64_t values = 0, hits = 0, mismatches = 0;
    for (const ClassCount& c : cls) {
        printf("class %-20s values=%llu hits=%llu (%.1f%%) mismatches=%llu\n", c.name, (unsigned long long)c.values, (unsigned long long)c.hits,
               c.values ? 100.0 * (double)c.hits / (double)c.values : 0.0, (unsigned long long)c.mismatches);
        values += c.values, hits += c.hits, mismatches += c.mismatches;
    }
    printf("exact path: values=%llu hits=%llu mismatches=%llu\n", (unsigned long long)values, (unsigned long long)hits,
           (unsigned long long)mismatches);
    CHECK(mismatches == 0, "%llu values of the exact path differ from std::to_chars", (unsigned long long)mismatches);
}

int main(int argc, char** argv) {
    const uint64_t per_class = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2600000ull;
    test_integers();
    test_float_table();
    test_strings();
    test_exact_path(per_class);
    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
