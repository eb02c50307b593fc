// tests/native/csv_host_test.cpp -- csv_number.hpp (the code the CSV kernels run) and csv_host.hpp on the CPU:
// the int64 edges, the float grammar and the boundary of the exact path, the exact values and the deferred
// conversion against strtod, the bool match, the class bits and the type rule, the quotes of a field, the header
// names, the argument checks in their order, the refusal of an OXH_CSV_STRING column at 2^31 bytes, the leases.
// Built by oxen_amd/build.py (build_host); the tests also build it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../oxen_amd/csrc/csv_host.hpp"

namespace num = oxh::csvnum;
namespace csv = oxh::csv;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// Every parser gets its text in a heap block of exactly its length: a read past the end is the sanitizer's.
struct Text {
    std::vector<uint8_t> b;
    explicit Text(const char* s) : b(s, s + std::strlen(s)) {}
    const uint8_t* p() const { return b.data(); }
    uint32_t n() const { return (uint32_t)b.size(); }
};

static uint32_t int_of(const char* s, int64_t& v) {
    const Text t(s);
    return num::parse_int64(t.p(), t.n(), v);
}

static uint32_t float_of(const char* s, uint64_t& m, int32_t& e, bool& neg) {
    const Text t(s);
    return num::parse_float(t.p(), t.n(), m, e, neg);
}

static uint64_t bits_of(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

static void ints() {
    int64_t v = 0;
    CHECK(int_of("9223372036854775807", v) == num::kIntValue && v == INT64_MAX);
    CHECK(int_of("9223372036854775808", v) == num::kIntOutOfRange);
    CHECK(int_of("-9223372036854775808", v) == num::kIntValue && v == INT64_MIN);
    CHECK(int_of("-9223372036854775809", v) == num::kIntOutOfRange);
    CHECK(int_of("+9223372036854775807", v) == num::kIntValue && v == INT64_MAX);
    CHECK(int_of("1000000000000000000", v) == num::kIntValue && v == 1000000000000000000ll);  // 19 digits
    CHECK(int_of("10000000000000000000", v) == num::kIntOutOfRange);                           // 20 digits
    CHECK(int_of("99999999999999999999999999999999999999", v) == num::kIntOutOfRange);
    CHECK(int_of("00000000000000000000000000000000000007", v) == num::kIntValue && v == 7);
    CHECK(int_of("+", v) == num::kIntNoMatch && int_of("-", v) == num::kIntNoMatch && int_of("", v) == num::kIntNoMatch);
    CHECK(int_of("-0", v) == num::kIntValue && v == 0);
    CHECK(int_of("+5", v) == num::kIntValue && v == 5);
    CHECK(int_of("1 ", v) == num::kIntNoMatch && int_of(" 1", v) == num::kIntNoMatch && int_of("1.0", v) == num::kIntNoMatch);
    CHECK(int_of("12a", v) == num::kIntNoMatch && int_of("99999999999999999999x", v) == num::kIntNoMatch);
}

static void exact_is_strtod(const char* s) {
    uint64_t m;
    int32_t e;
    bool neg;
    const uint32_t kind = float_of(s, m, e, neg);
    if (kind != num::kFloatExact) {
        std::fprintf(stderr, "not exact: %s (%u)\n", s, kind);
        ++failures;
        return;
    }
    const double got = num::exact_value(m, e, neg, kPow10), want = std::strtod(s, nullptr);
    if (bits_of(got) != bits_of(want)) {
        std::fprintf(stderr, "%s: %a, strtod %a\n", s, got, want);
        ++failures;
    }
}

static void floats() {
    uint64_t m;
    int32_t e;
    bool neg;
    // the grammar
    for (const char* s : {"1", "1.", ".5", "1.5", "+1.5", "-1.5", "1e5", "1E5", "1e+5", "1e-5", "1.e5", ".5e5", "0", "-0", "0.0", "000.000",
                          "1e0005", "inf", "INF", "-Infinity", "+iNfInItY", "nan", "NaN", "-nan"})
        CHECK(float_of(s, m, e, neg) != num::kFloatNoMatch);
    for (const char* s : {"", "+", "-", ".", "+.", "e5", ".e5", "1e", "1e+", "1e-", "1e5.", "1.5.2", "1 ", " 1", "1f", "0x10", "infi", "infinit",
                          "infinityy", "na", "nane", "1_000", "--1", "1e5e5", "1,5"})
        CHECK(float_of(s, m, e, neg) == num::kFloatNoMatch);
    CHECK(float_of("inf", m, e, neg) == num::kFloatInf && !neg);
    CHECK(float_of("-INFINITY", m, e, neg) == num::kFloatInf && neg);
    CHECK(float_of("-NaN", m, e, neg) == num::kFloatNan && neg);
    // the boundary of the exact path
    CHECK(float_of("9007199254740992", m, e, neg) == num::kFloatExact && m == (1ull << 53) && e == 0);   // 2^53
    CHECK(float_of("9007199254740993", m, e, neg) == num::kFloatDeferred);                               // 2^53 + 1
    CHECK(float_of("1e22", m, e, neg) == num::kFloatExact && m == 1 && e == 22);
    CHECK(float_of("1e23", m, e, neg) == num::kFloatDeferred);
    CHECK(float_of("1e-22", m, e, neg) == num::kFloatExact && e == -22);
    CHECK(float_of("1e-23", m, e, neg) == num::kFloatDeferred);
    CHECK(float_of("0.0000000000000000000001", m, e, neg) == num::kFloatExact && m == 1 && e == -22);
    CHECK(float_of("0.00000000000000000000001", m, e, neg) == num::kFloatDeferred);
    CHECK(float_of("1234567890123456789", m, e, neg) == num::kFloatDeferred && m == 1234567890123456789ull);  // 19 digits, above 2^53
    CHECK(float_of("12345678901234567890", m, e, neg) == num::kFloatDeferred);                               // 20 digits
    CHECK(float_of("1000000000000000000000", m, e, neg) == num::kFloatDeferred);                             // 22 digits, zeros or not
    CHECK(float_of("0000000000000000000000001.5", m, e, neg) == num::kFloatExact && m == 15 && e == -1);      // leading zeros are none
    CHECK(float_of("0e99999999999", m, e, neg) == num::kFloatExact && m == 0);
    CHECK(float_of("1e99999999999", m, e, neg) == num::kFloatDeferred);
    CHECK(num::exact_path(1ull << 53, 22) && !num::exact_path((1ull << 53) + 1, 0) && !num::exact_path(1, 23) && !num::exact_path(1, -23));
    for (const char* s : {"1", "1.", ".5", "0.1", "-0.1", "3.14159", "123456.789", "1e22", "1e-22", "9007199254740992", "9007199254740991e22",
                          "9007199254740991e-22", "0.3", "2.5e-5", "+7.25", "-0", "0e999999", "-0.0e-999999", "450359962737049.5"})
        exact_is_strtod(s);
    CHECK(bits_of(num::exact_value(0, -100000, true, kPow10)) == num::kSignBit);
    // the deferred conversion against strtod
    for (const char* s : {"9007199254740993", "1e23", "1e-23", "0.1e-30", "1.7976931348623157e308", "1.7976931348623159e308", "1e400", "-1e400",
                          "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "1e-400", "-1e-400", "2.2250738585072011e-308",
                          "123456789012345678901234567890", "0.1234567890123456789012345", "+1e23", "-1e23", "1.e23", ".1e40",
                          "8.41e21", "9.5367431640625e-07", "3.141592653589793238462643383279", "1e99999999999", "1e-99999999999"}) {
        const double got = csv::convert_deferred(s, std::strlen(s)), want = std::strtod(s, nullptr);
        if (bits_of(got) != bits_of(want)) {
            std::fprintf(stderr, "deferred %s: %a, strtod %a\n", s, got, want);
            ++failures;
        }
    }
}

static void bools_and_classes() {
    bool b = false;
    const Text t("TrUe"), f("FALSE"), x("truee"), y("fals"), z("");
    CHECK(num::parse_bool(t.p(), t.n(), b) && b);
    CHECK(num::parse_bool(f.p(), f.n(), b) && !b);
    CHECK(!num::parse_bool(x.p(), x.n(), b) && !num::parse_bool(y.p(), y.n(), b) && !num::parse_bool(z.p(), 0, b));
    auto bits = [](const char* s) {
        const Text c(s);
        return num::class_bits(c.p(), c.n());
    };
    CHECK(bits("") == num::kAllOk);
    CHECK(bits("12") == (num::kIntOk | num::kFloatOk));
    CHECK(bits("99999999999999999999") == num::kFloatOk);  // not an int64: a float column
    CHECK(bits("1.5") == num::kFloatOk && bits("nan") == num::kFloatOk);
    CHECK(bits("true") == num::kBoolOk && bits("abc") == 0 && bits(" 1") == 0);
    CHECK(csv::type_of_bits(num::kAllOk, true) == OXH_CSV_STRING);
    CHECK(csv::type_of_bits(num::kIntOk | num::kFloatOk, false) == OXH_CSV_INT64);
    CHECK(csv::type_of_bits(num::kFloatOk, false) == OXH_CSV_FLOAT64);
    CHECK(csv::type_of_bits(num::kBoolOk, false) == OXH_CSV_BOOL);
    CHECK(csv::type_of_bits(0, false) == OXH_CSV_STRING);
}

static void fields() {
    auto value = [](const char* s, uint32_t quote) {
        const Text t(s);
        return csv::field_value(t.p(), t.n(), quote);
    };
    CHECK(value("abc", '"') == "abc" && value("\"abc\"", '"') == "abc" && value("\"\"", '"') == "" && value("\"", '"') == "\"");
    CHECK(value("\"a\"\"b\"", '"') == "a\"b" && value("\"a\"\"\"b\"", '"') == "a\"\"b" && value("\"a\"b\"", '"') == "a\"b");
    CHECK(value("\"\"\"\"", '"') == "\"" && value("\"\"\"\"\"\"", '"') == "\"\"");
    CHECK(value("\"abc\"", OXH_CSV_NO_QUOTE) == "\"abc\"" && value("a\"b", '"') == "a\"b" && value("'x'", '\'') == "x");
    const Text rec("id,\"na\"\"me\",\"x,y\"\r");  // a header record that starts at byte 100 of its buffer
    const uint32_t ends[3] = {102, 111, 118};
    std::vector<uint8_t> names;
    std::vector<uint64_t> offsets;
    csv::header_names(rec.p(), 100, ends, 3, '"', names, offsets);
    CHECK(std::string(names.begin(), names.end()) == "idna\"mex,y");
    CHECK(offsets == (std::vector<uint64_t>{0, 2, 7, 10}));
}

static void arguments() {
    uint8_t byte = 0;
    void* out = nullptr;
    uint64_t stats[8] = {};
    auto err = [&](const uint8_t* b, uint64_t n, uint32_t sep, uint32_t quote, uint32_t flags, void** o, const uint64_t* s) {
        return csv::open_error(b, n, sep, quote, flags, o, s);
    };
    CHECK(err(&byte, 1, ',', '"', 1, &out, stats).empty() && err(nullptr, 0, '\t', OXH_CSV_NO_QUOTE, 0, &out, stats).empty());
    // each refusal comes before the ones after it
    CHECK(err(nullptr, 1ull << 32, 256, 257, 2, nullptr, nullptr).find("separator is not one byte") != std::string::npos);
    CHECK(err(nullptr, 1ull << 32, ',', 257, 2, nullptr, nullptr).find("quote is neither") != std::string::npos);
    CHECK(err(nullptr, 1ull << 32, '\n', '\n', 2, nullptr, nullptr).find("separator is a line end") != std::string::npos);
    CHECK(err(nullptr, 1ull << 32, ',', '\r', 2, nullptr, nullptr).find("quote is a line end") != std::string::npos);
    CHECK(err(nullptr, 1ull << 32, ',', ',', 2, nullptr, nullptr).find("quote is the separator") != std::string::npos);
    CHECK(err(nullptr, 1ull << 32, ',', '"', 2, nullptr, nullptr).find("unknown flags") != std::string::npos);
    CHECK(err(nullptr, 1ull << 32, ',', '"', 1, nullptr, nullptr).find("2^32") != std::string::npos);
    CHECK(err(nullptr, (1ull << 32) - 1, ',', '"', 1, nullptr, nullptr).find("bytes is NULL") != std::string::npos);
    CHECK(err(&byte, 1, ',', '"', 1, nullptr, nullptr).find("out is NULL") != std::string::npos);
    CHECK(err(&byte, 1, ',', '"', 1, &out, nullptr).find("stats8 is NULL") != std::string::npos);

    const uint32_t idx[2] = {0, 2}, types[2] = {OXH_CSV_INT64, OXH_CSV_STRING};
    uint64_t cap[2] = {80, 5}, vb[2], st[8];
    uint64_t cells[10];
    uint32_t offs[11];
    uint8_t val[2], chars[5];
    void* values[2] = {cells, chars};
    void* offsets[2] = {nullptr, offs};
    uint8_t* validity[2] = {val, val};
    csv::ColumnsArgs a{10, 3, 2, idx, types, cap, values, offsets, validity, vb, st};
    CHECK(csv::columns_error(a).empty());
    csv::ColumnsArgs m = a;
    m.values = nullptr, m.offsets = nullptr, m.validity = nullptr, m.value_capacity = nullptr;
    CHECK(csv::columns_error(m).empty());  // the measure
    csv::ColumnsArgs b = a;
    b.col_idx = nullptr;
    CHECK(csv::columns_error(b).find("col_idx or types is NULL") != std::string::npos);
    const uint32_t far[2] = {0, 3}, odd[2] = {OXH_CSV_INT64, 6}, none[2] = {0, 4};
    b = a, b.col_idx = far, b.types = odd;
    CHECK(csv::columns_error(b).find("names column 3 of 3") != std::string::npos);
    b = a, b.types = odd, b.stats4 = nullptr;
    CHECK(csv::columns_error(b).find("unknown type 6") != std::string::npos);
    b = a, b.types = none;
    CHECK(csv::columns_error(b).find("unknown type 0") != std::string::npos);
    b = a, b.stats4 = nullptr, b.offsets = nullptr;
    CHECK(csv::columns_error(b).find("value_bytes or stats4 is NULL") != std::string::npos);
    b = a, b.offsets = nullptr, b.value_capacity = nullptr;
    CHECK(csv::columns_error(b).find("only some of") != std::string::npos);
    b = a, b.value_capacity = nullptr;
    CHECK(csv::columns_error(b).find("value_capacity is NULL") != std::string::npos);
    uint8_t* no_validity[2] = {val, nullptr};
    b = a, b.validity = no_validity;
    CHECK(csv::columns_error(b).find("selection 1 has no validity") != std::string::npos);
    void* no_offsets[2] = {nullptr, nullptr};
    b = a, b.offsets = no_offsets;
    CHECK(csv::columns_error(b).find("string column without offsets") != std::string::npos);
    void* no_values[2] = {nullptr, chars};
    b = a, b.values = no_values;
    CHECK(csv::columns_error(b).find("selection 0 has no values") != std::string::npos);
    uint64_t small[2] = {79, 5};
    b = a, b.value_capacity = small;
    CHECK(csv::columns_error(b).find("below the 80 bytes") != std::string::npos);
    void* odd_values[2] = {(uint8_t*)cells + 4, chars};
    b = a, b.values = odd_values;
    CHECK(csv::columns_error(b).find("values is not 8-byte aligned") != std::string::npos);
    void* odd_offsets[2] = {nullptr, (uint8_t*)offs + 2};
    b = a, b.offsets = odd_offsets;
    CHECK(csv::columns_error(b).find("offsets is not aligned") != std::string::npos);
    b = a, b.nrows = 0, b.validity = no_validity;
    CHECK(csv::columns_error(b).empty());  // no rows: nothing is written, nothing is needed

    // an OXH_CSV_STRING column is refused at 2^31 bytes by its measure alone; OXH_CSV_STRING64 is not
    CHECK(csv::string_bytes_error(OXH_CSV_STRING, (1ull << 31) - 1, false, 0).empty());
    CHECK(csv::string_bytes_error(OXH_CSV_STRING, 1ull << 31, false, 0).find("OXH_CSV_STRING64") != std::string::npos);
    CHECK(csv::string_bytes_error(OXH_CSV_STRING64, 1ull << 31, false, 0).empty());
    CHECK(csv::string_bytes_error(OXH_CSV_STRING64, 11, true, 10).find("value_capacity 10") != std::string::npos);
    CHECK(csv::string_bytes_error(OXH_CSV_STRING, 10, true, 10).empty());
    CHECK(csv::fixed_value_bytes(OXH_CSV_BOOL, 9) == 2 && csv::fixed_value_bytes(OXH_CSV_FLOAT64, 9) == 72);
}

static void leases() {
    CHECK(csv::tiles_of(0, 1) == 1 && csv::tiles_of(0, csv::kTileBytes - 1) == 1 && csv::tiles_of(0, csv::kTileBytes) == 2);
    CHECK(csv::tiles_of(15, csv::kTileBytes - 16) == 1 && csv::tiles_of(15, csv::kTileBytes - 15) == 2);
    const csv::IndexLease a(5000);
    CHECK(a.ctrl == 0 && a.quotes == 256 && a.total % 256 == 0 && a.rec_sums + csv::align256((csv::scan_tiles_of(5000) + 1) * 8) == a.total);
    CHECK(a.quote_scan >= a.quotes + 5000 * 4 && a.delims >= a.quote_scan + 5000 * 8 && a.rec_scan >= a.recs + 5000 * 4);
    const csv::RowMapLease r(65);
    CHECK(r.mask == 256 && r.counts == 512 && r.bases == 768 && r.sums == 1024 && r.total == 1280);
    const uint32_t types[3] = {OXH_CSV_FLOAT64, OXH_CSV_STRING, OXH_CSV_FLOAT64};
    const csv::ColumnsLease c(1000, 3, types, true);
    CHECK(c.lens >= 3 * 64 + csv::kCtrlBytes && c.len_scan >= c.lens + 4000 && c.sums >= c.len_scan + 8000);
    CHECK(c.defer_mask[0] && c.defer_mask[2] > c.defer_counts[0] && !c.defer_mask[1] && c.total >= c.defer_counts[2] + 16 * 4);
}

int main() {
    ints();
    floats();
    bools_and_classes();
    fields();
    arguments();
    leases();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
