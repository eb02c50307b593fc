// tests/native/json_write_host_test.cpp -- the JSON writer's text functions on the CPU (oxen_amd/csrc/json_text.hpp,
// the code the kernels of json_write.hip compile): the width and the put of all 256 byte values against a table
// written out here, the escaped length against the put on random spans of a fixed seed (and the put into a room too small), the float rule (non-finite
// values are null), and keys that need escaping.
// Build: g++ -std=c++17 -O2 -Wall -o json_write_host_test json_write_host_test.cpp   (oxen_amd/build.py does)
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../oxen_amd/csrc/json_text.hpp"

namespace j = oxh::jsontext;
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

// The rule, written out a second time: what byte c is inside a JSON string.
static std::string expected_byte(unsigned c) {
    switch (c) {
        case '"': return "\\\"";
        case '\\': return "\\\\";
        case 0x08: return "\\b";
        case 0x0C: return "\\f";
        case 0x0A: return "\\n";
        case 0x0D: return "\\r";
        case 0x09: return "\\t";
        default: break;
    }
    if (c < 0x20) {
        char buf[8];
        snprintf(buf, sizeof buf, "\\u%04x", c);
        return buf;
    }
    return std::string(1, (char)c);
}

static void test_every_byte() {
    for (unsigned c = 0; c < 256; ++c) {
        const std::string want = expected_byte(c);
        uint8_t buf[8];
        memset(buf, '#', sizeof buf);
        const uint32_t w = j::byte_width(c);
        CHECK(w == want.size(), "byte_width(0x%02x) = %u, not %zu", c, w, want.size());
        CHECK(j::byte_put(c, buf) == w, "byte_put(0x%02x) returns another width", c);
        CHECK(std::string((const char*)buf, w) == want, "byte_put(0x%02x)", c);
        CHECK(buf[w] == '#', "byte_put(0x%02x) wrote behind its width", c);
        CHECK(w == 1 || w == 2 || w == 6, "a width of %u", w);
    }
    CHECK(j::byte_width(0x7F) == 1 && j::byte_width('/') == 1 && j::byte_width(0x80) == 1 && j::byte_width(0xFF) == 1, "bytes copied as they are");
    CHECK(expected_byte(0x1f) == "\\u001f" && expected_byte(0x0b) == "\\u000b", "lowercase hex");
}

static std::string string_text(const std::vector<uint8_t>& raw) {
    const uint64_t l = j::escaped_len(raw.data(), raw.size());
    std::vector<uint8_t> buf(l + 3, '#');
    CHECK(j::string_put(raw.data(), raw.size(), buf.data(), l + 2) == l + 2, "string_put: the length is not escaped_len + 2");
    CHECK(buf[l + 2] == '#', "string_put wrote behind its length");
    for (uint64_t room = 0; room < l + 2 && room < 12; ++room) {  // a room too small: refused, nothing behind it is written
        std::vector<uint8_t> tight(room + 8, '#');
        CHECK(j::string_put(raw.data(), raw.size(), tight.data(), room) == room + 1, "string_put fits a room of %llu", (unsigned long long)room);
        for (uint64_t b = room; b < room + 8; ++b) CHECK(tight[b] == '#', "string_put wrote behind a room of %llu", (unsigned long long)room);
    }
    if (l + 2 > 12) {
        std::vector<uint8_t> tight(l + 1 + 8, '#');
        CHECK(j::string_put(raw.data(), raw.size(), tight.data(), l + 1) == l + 2, "string_put fits a room one byte short");
        for (uint64_t b = l + 1; b < l + 9; ++b) CHECK(tight[b] == '#', "string_put wrote behind a room one byte short");
    }
    return std::string((const char*)buf.data(), l + 2);
}

static void test_spans(uint64_t rounds) {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        return state;
    };
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t n = next() % 200;
        const unsigned cls = (unsigned)(next() % 4);  // any byte, mostly controls, ASCII text, nothing to escape
        std::vector<uint8_t> raw(n);
        for (auto& b : raw) {
            const uint64_t v = next();
            b = cls == 0 ? (uint8_t)v : cls == 1 ? (uint8_t)(v % 0x24) : cls == 2 ? (uint8_t)(0x20 + v % 0x60) : (uint8_t)('a' + v % 26);
        }
        std::string want = "\"";
        for (uint8_t b : raw) want += expected_byte(b);
        want += "\"";
        CHECK(string_text(raw) == want, "a span of %llu bytes of class %u", (unsigned long long)n, cls);
        if (cls == 3) CHECK(j::escaped_len(raw.data(), n) == n, "a plain span widened");
    }
    CHECK(string_text({}) == "\"\"", "the empty string");
    std::vector<uint8_t> all(256);
    for (unsigned c = 0; c < 256; ++c) all[c] = (uint8_t)c;
    CHECK(j::escaped_len(all.data(), 256) == 256 + 7 + 27 * 5, "all 256 bytes: %llu", (unsigned long long)j::escaped_len(all.data(), 256));
}

static std::string float_text(double v) {
    uint64_t bits;
    memcpy(&bits, &v, 8);
    const t::FloatForm f = t::float_form(bits, kPow10);
    uint8_t buf[40];
    memset(buf, '#', sizeof buf);
    if (f.kind == t::kFormDeferred) {
        t::deferred_slot(bits, buf);
        return std::string((const char*)buf, buf[t::kDeferSlot - 1]);
    }
    const uint32_t n = j::float_form_text(f, nullptr);
    CHECK(j::float_form_text(f, buf) == n && buf[n] == '#', "float_form_text: measured and written differ");
    return std::string((const char*)buf, n);
}

static void test_floats() {
    const double inf = 1.0 / 0.0;
    uint64_t payload = 0x7FF80000DEADBEEFull, negative = 0xFFF0000000000001ull;
    double nan1, nan2;
    memcpy(&nan1, &payload, 8), memcpy(&nan2, &negative, 8);
    CHECK(float_text(inf) == "null" && float_text(-inf) == "null" && float_text(nan1) == "null" && float_text(nan2) == "null", "non-finite");
    CHECK(float_text(0.0) == "0.0" && float_text(-0.0) == "-0.0", "the zeros");
    CHECK(float_text(12.5) == "12.5" && float_text(1e-6) == "1e-6" && float_text(1e15) == "1000000000000000.0", "finite values");
    CHECK(float_text(0.1 + 0.2) == "0.30000000000000004" && float_text(5e-324) == "5e-324", "deferred values");
}

static std::string key(const char* name, size_t n, bool first, bool* escaped = nullptr) {
    std::vector<uint8_t> text;
    const bool e = j::key_text((const uint8_t*)name, n, first, text);
    if (escaped) *escaped = e;
    return std::string(text.begin(), text.end());
}

static void test_keys() {
    bool e;
    CHECK(key("a", 1, true, &e) == "{\"a\":" && !e, "the first key");
    CHECK(key("b", 1, false, &e) == ",\"b\":" && !e, "a later key");
    CHECK(key("", 0, true, &e) == "{\"\":" && !e, "the empty name");
    CHECK(key(nullptr, 0, false, &e) == ",\"\":" && !e, "the empty name without bytes");
    CHECK(key("q\"b\\c\x01\n", 7, false, &e) == ",\"q\\\"b\\\\c\\u0001\\n\":" && e, "a name that needs escaping");
    CHECK(key("\xc3\xa9/\x7f", 4, true, &e) == "{\"\xc3\xa9/\x7f\":" && !e, "non-ASCII, '/' and 0x7F stay");
    const std::string wide(300, 'w');
    CHECK(key(wide.data(), 300, false) == ",\"" + wide + "\":", "a 300-byte name");
}

int main(int argc, char** argv) {
    const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 200000;
    test_every_byte();
    test_spans(rounds);
    test_floats();
    test_keys();
    if (g_failures) {
        fprintf(stderr, "%d failures\n", g_failures);
        return 1;
    }
    printf("json text: spans=%llu\nok\n", (unsigned long long)rounds);
    return 0;
}
