// tests/native/jsonl_host_test.cpp -- jsonl_text.hpp (the code the JSON Lines kernels run) and jsonl_host.hpp on
// the CPU: the cell grammar, the unescape step with its surrogate rules, the key compare, the well-formed-record
// rule, the class bits, the argument checks in their order, the names from key text, the leases; and the three
// carries -- folded over 16-byte lanes, 64-lane waves, 4-wave tiles and the tiles in order, at every misalignment,
// as the kernels fold them -- against a byte-by-byte state machine over buffers dense in backslashes, quotes,
// brackets and newlines, runs of backslashes that cover whole tiles included.
// Built by oxen_amd/build.py (build_host); the tests also build it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../oxen_amd/csrc/jsonl_host.hpp"

namespace jl = oxh::jsonl;
namespace num = oxh::csvnum;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const std::string BS = "\\";
static const std::string U = BS + "u";  // the two bytes that start a unicode escape

// Every parser gets its text in a heap block of exactly its length: a read past the end is the sanitizer's.
struct Text {
    std::vector<uint8_t> b;
    explicit Text(const std::string& s) : b(s.begin(), s.end()) {}
    const uint8_t* p() const { return b.data(); }
    uint32_t n() const { return (uint32_t)b.size(); }
};

static uint32_t kind_of(const std::string& s, uint32_t* len = nullptr) {
    const Text t(s);
    uint32_t l = 0;
    const uint32_t k = jl::cell_kind(t.p(), t.n(), l);
    if (len) *len = l;
    return k;
}

// "-": not a string token.
static std::string unescaped(const std::string& s) {
    const Text t(s);
    uint32_t len = 0;
    if (!jl::string_token(t.p(), t.n(), len)) return "-";
    std::vector<uint8_t> out(len + 1, 0xEE);
    CHECK(jl::unescape_copy(t.p(), t.n(), out.data(), len) == len);
    CHECK(out[len] == 0xEE);
    CHECK(len + 2 <= t.n());  // never longer than the raw text
    return std::string(out.begin(), out.begin() + len);
}

static bool key_is(const std::string& tok, const std::string& name) {
    const Text t(tok), n(name);
    return jl::key_equals(t.p(), t.n(), n.p(), n.n());
}

static void test_grammar() {
    CHECK(kind_of("0") == jl::kInteger && kind_of("-0") == jl::kInteger && kind_of("12345678901234567890") == jl::kInteger);
    CHECK(kind_of("1.5") == jl::kNumber && kind_of("-1e5") == jl::kNumber && kind_of("1E+5") == jl::kNumber && kind_of("0.0e-0") == jl::kNumber);
    CHECK(kind_of("1e400") == jl::kNumber);
    for (const char* bad : {"01", "1.", ".5", "-", "+1", "1e", "1e+", "1.e5", "0x1", "1 2", "--1", "1.5.2", "Infinity", "NaN", "-inf"})
        CHECK(kind_of(bad) == jl::kUnparsable);
    CHECK(kind_of("true") == jl::kTrue && kind_of("false") == jl::kFalse && kind_of("null") == jl::kNull);
    for (const char* bad : {"tru", "True", "truee", "nul", "NULL", "fals", "x", "'a'"}) CHECK(kind_of(bad) == jl::kUnparsable);
    CHECK(kind_of("{}") == jl::kNested && kind_of("[1,2]") == jl::kNested && kind_of("[}") == jl::kUnparsable && kind_of("{]") == jl::kUnparsable);
    CHECK(kind_of("{\"a\":1} x") == jl::kUnparsable && kind_of("[") == jl::kUnparsable);
    uint32_t len = 0;
    CHECK(kind_of("\"\"", &len) == jl::kString && len == 0);
    CHECK(kind_of("\"abc\"", &len) == jl::kString && len == 3);
    CHECK(kind_of("\"a\" \"b\"") == jl::kUnparsable && kind_of("\"abc") == jl::kUnparsable && kind_of("\"") == jl::kUnparsable);
    CHECK(kind_of("\"a\tb\"") == jl::kUnparsable);               // a raw tab
    CHECK(kind_of("\"a" + BS + "x\"") == jl::kUnparsable);       // no such escape
    CHECK(kind_of("\"a" + BS + "\"") == jl::kUnparsable);        // an odd trailing backslash: the quote is escaped
    CHECK(kind_of("\"a" + BS + BS + "\"", &len) == jl::kString && len == 2);
    // the class bits
    auto bits = [](const std::string& s) {
        const Text t(s);
        return jl::class_bits(t.p(), t.n());
    };
    CHECK(bits("null") == num::kAllOk && bits("12") == (num::kIntOk | num::kFloatOk) && bits("9223372036854775808") == num::kFloatOk);
    CHECK(bits("-9223372036854775808") == (num::kIntOk | num::kFloatOk) && bits("1.0") == num::kFloatOk && bits("true") == num::kBoolOk);
    CHECK(bits("\"1\"") == 0 && bits("[1]") == 0 && bits("tru") == 0);
    CHECK(jl::type_of_bits(num::kAllOk, true) == OXH_CSV_STRING && jl::type_of_bits(3, false) == OXH_CSV_INT64 &&
          jl::type_of_bits(2, false) == OXH_CSV_FLOAT64 && jl::type_of_bits(4, false) == OXH_CSV_BOOL && jl::type_of_bits(0, false) == OXH_CSV_STRING);
}

static void test_unescape() {
    CHECK(unescaped("\"plain\"") == "plain");
    CHECK(unescaped("\"" + BS + "\"" + BS + BS + BS + "/" + BS + "b" + BS + "f" + BS + "n" + BS + "r" + BS + "t\"") == "\"\\/\b\f\n\r\t");
    CHECK(unescaped("\"" + U + "0041" + U + "00e9" + U + "20AC\"") == "A\xC3\xA9\xE2\x82\xAC");
    CHECK(unescaped("\"" + U + "0000\"") == std::string(1, '\0'));
    CHECK(unescaped("\"" + U + "d83d" + U + "DE00\"") == "\xF0\x9F\x98\x80");  // a surrogate pair: 12 bytes to 4
    CHECK(unescaped("\"" + U + "d83d\"") == "-" && unescaped("\"" + U + "de00\"") == "-");      // lone surrogates
    CHECK(unescaped("\"" + U + "d83dx" + U + "de00\"") == "-" && unescaped("\"" + U + "d83d" + U + "0041\"") == "-");
    CHECK(unescaped("\"" + U + "d83d" + BS + "n\"") == "-" && unescaped("\"" + U + "d83d" + U + "de0\"") == "-");
    CHECK(unescaped("\"" + U + "00g1\"") == "-" && unescaped("\"" + U + "12\"") == "-" && unescaped("\"" + U + "\"") == "-");
    CHECK(unescaped("\"tr\xC3\xA9s \xFF\"") == "tr\xC3\xA9s \xFF");            // bytes at or above 0x80 as they are
    // the key compare goes through the same step
    CHECK(key_is("\"ab\"", "ab") && key_is("\"a" + U + "0062\"", "ab") && !key_is("\"ab\"", "abc") && !key_is("\"abc\"", "ab"));
    CHECK(!key_is("\"a" + BS + "x\"", "ax") && key_is("\"\"", "") && !key_is("ab", "ab"));
    // a copy with less room than the text stops at the room
    const Text t("\"abcdef\"");
    std::vector<uint8_t> small(3, 0xEE);
    CHECK(jl::unescape_copy(t.p(), t.n(), small.data(), 2) == 6 && small[0] == 'a' && small[1] == 'b' && small[2] == 0xEE);
}

// ---------------------------------------------------------------- the index, two ways
struct Index {
    std::vector<uint32_t> ends, rec_end;
    bool operator==(const Index& o) const { return ends == o.ends && rec_end == o.rec_end; }
};

// Byte by byte, as the header states the rules.
static Index index_naive(const std::vector<uint8_t>& d) {
    Index x;
    bool escaped = false, inside = false;
    int64_t depth = 0;
    const uint32_t n = (uint32_t)d.size();
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t c = d[i];
        const bool was = escaped;
        escaped = c == '\\' && !was;
        if (c == '\n') {
            x.rec_end.push_back((uint32_t)x.ends.size());
            x.ends.push_back(i);
            escaped = inside = false, depth = 0;
        } else if (c == '"' && !was) {
            inside = !inside;
        } else if (!inside) {
            if (c == '{' || c == '[') {
                if (depth == 0) x.ends.push_back(i);
                ++depth;
            } else if (c == '}' || c == ']') {
                if (depth <= 1) x.ends.push_back(i);
                --depth;
            } else if ((c == ':' || c == ',') && depth == 1) {
                x.ends.push_back(i);
            }
        }
    }
    if (n && d[n - 1] != '\n') {
        x.rec_end.push_back((uint32_t)x.ends.size());
        x.ends.push_back(n);
    }
    return x;
}

struct Masks {
    uint32_t bs = 0, q = 0, nl = 0, op = 0, cl = 0, co = 0;
};

template <class T>
static std::vector<T> exclusive(const std::vector<T>& v, T& total) {
    std::vector<T> out(v.size());
    T run = T::identity();
    for (size_t i = 0; i < v.size(); ++i) out[i] = run, run = T::compose(run, v[i]);
    total = run;
    return out;
}

// A fold in the kernels' grouping: the lanes of a wave, the waves of a tile, the tiles in order -- each level
// folded on its own and composed with the levels above, so a compose that is not associative shows.
template <class T>
static std::vector<T> exclusive_grouped(const std::vector<T>& lanes) {
    const size_t n = lanes.size();
    std::vector<T> waves, tiles, out(n);
    for (size_t w = 0; w * 64 < n; ++w) {
        T t = T::identity();
        for (size_t i = w * 64; i < std::min(n, w * 64 + 64); ++i) t = T::compose(t, lanes[i]);
        waves.push_back(t);
    }
    for (size_t t = 0; t * 4 < waves.size(); ++t) {
        T s = T::identity();
        for (size_t w = t * 4; w < std::min(waves.size(), t * 4 + 4); ++w) s = T::compose(s, waves[w]);
        tiles.push_back(s);
    }
    T tile_total, unused;
    const std::vector<T> tile_in = exclusive(tiles, tile_total);
    for (size_t i = 0; i < n; ++i) {
        const size_t w = i / 64, t = w / 4;
        T in_wave = T::identity(), in_tile = T::identity();
        for (size_t k = w * 64; k < i; ++k) in_wave = T::compose(in_wave, lanes[k]);
        for (size_t k = t * 4; k < w; ++k) in_tile = T::compose(in_tile, waves[k]);
        out[i] = T::compose(tile_in[t], T::compose(in_tile, in_wave));
    }
    (void)unused;
    return out;
}

static Index index_by_carries(const std::vector<uint8_t>& d, uint32_t mis) {
    const uint64_t n = d.size(), lo = mis, hi = mis + n;
    const uint64_t nlanes = (hi + 1 + 15) / 16;
    std::vector<Masks> m(nlanes);
    for (uint64_t at = lo; at < hi; ++at) {
        const uint8_t c = d[at - lo];
        Masks& x = m[at / 16];
        const uint32_t j = at % 16;
        x.bs |= (uint32_t)(c == '\\') << j, x.q |= (uint32_t)(c == '"') << j, x.nl |= (uint32_t)(c == '\n') << j;
        x.op |= (uint32_t)((c | 0x20) == '{') << j, x.cl |= (uint32_t)((c | 0x20) == '}') << j, x.co |= (uint32_t)(c == ':' || c == ',') << j;
    }
    std::vector<jl::EscCarry> esc(nlanes);
    for (uint64_t l = 0; l < nlanes; ++l) esc[l] = jl::esc_of_lane(m[l].bs);
    const std::vector<jl::EscCarry> esc_before = exclusive_grouped(esc);
    std::vector<uint32_t> uq(nlanes);
    std::vector<jl::LineCarry<int64_t>> line(nlanes);
    for (uint64_t l = 0; l < nlanes; ++l) {
        uq[l] = m[l].q & ~jl::escaped_mask(m[l].bs, jl::esc_in(esc_before[l], 0));
        const jl::LineCarry<int32_t> c = jl::line_of_lane(uq[l], m[l].nl, m[l].op, m[l].cl);
        line[l] = jl::LineCarry<int64_t>{c.reset, c.par, c.d0, c.d1};
    }
    const std::vector<jl::LineCarry<int64_t>> before = exclusive_grouped(line);
    Index x;
    for (uint64_t l = 0; l < nlanes; ++l) {
        uint32_t delim = jl::kept_of_lane(uq[l], m[l].nl, m[l].op, m[l].cl, m[l].co, before[l].par, before[l].d0) | m[l].nl, rec = m[l].nl;
        const uint64_t v0 = l * 16;
        if (hi >= v0 && hi < v0 + 16 && n && d[n - 1] != '\n') delim |= 1u << (hi - v0), rec |= 1u << (hi - v0);
        for (uint32_t j = 0; j < 16; ++j) {
            if (!((delim >> j) & 1)) continue;
            if ((rec >> j) & 1) x.rec_end.push_back((uint32_t)x.ends.size());
            x.ends.push_back((uint32_t)(v0 + j - lo));
        }
    }
    return x;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static void test_carries() {
    // the escaped mask of every 16 bytes of backslashes, both carries, against a walk
    for (uint32_t bs = 0; bs < 65536; bs += 7)
        for (uint32_t carry = 0; carry < 2; ++carry) {
            uint32_t want = 0, e = carry;
            for (uint32_t j = 0; j < 16; ++j) {
                if (e) want |= 1u << j;
                e = ((bs >> j) & 1) && !e;
            }
            CHECK(jl::escaped_mask(bs, carry) == want);
        }
    const char alphabet[] = "\\\\\\\"\"{}[]:,\n ax";
    for (int round = 0; round < 60; ++round) {
        const uint32_t n = 1 + rnd() % 20000;
        std::vector<uint8_t> d(n);
        for (auto& c : d) c = (uint8_t)alphabet[rnd() % (sizeof alphabet - 1)];
        if (round % 3 == 0) {  // a run of backslashes over whole tiles, either parity, then a quote
            const uint32_t from = rnd() % n, len = std::min<uint32_t>(n - from, 4096 * (1 + rnd() % 3) + rnd() % 3);
            std::memset(d.data() + from, '\\', len);
            if (from + len < n) d[from + len] = '"';
        }
        if (round % 5 == 0) std::replace(d.begin(), d.end(), (uint8_t)'\n', (uint8_t)' ');  // one line longer than four tiles
        const Index want = index_naive(d);
        for (uint32_t mis : {0u, 1u, 7u, 15u}) CHECK(index_by_carries(d, mis) == want);
    }
    for (const std::string& s : {std::string(""), std::string("\n"), std::string("\n\n\n"), std::string("{}"), std::string(8192, '\\'),
                                std::string(4096, '\\') + "\"{", std::string(4095, '\\') + "\"{"}) {
        const std::vector<uint8_t> d(s.begin(), s.end());
        for (uint32_t mis = 0; mis < 16; ++mis) CHECK(index_by_carries(d, mis) == index_naive(d));
    }
}

// The well-formed rule over a line's own kept positions.
static bool well_formed(const std::string& line) {
    const std::vector<uint8_t> d(line.begin(), line.end());
    const Index x = index_naive(d);
    if (x.rec_end.size() != 1) return false;
    return jl::record_well_formed(d.data(), 0, (uint32_t)d.size(), x.ends.data(), x.rec_end[0]);
}

static void test_records() {
    for (const char* good : {"{}", " { } \r", "{\"a\":1}", "{\"a\": [1,{\"b\":\"}\"}] , \"c\" :null}", "{\"a\":\"x,y:z\"}", "{\"a\":[}}", "{\"a\":tru}"})
        CHECK(well_formed(good));
    for (const char* bad : {"{\"a\":1,}", "{\"a\" 1}", "{\"a\":}", "{:1}", "{\"a\":1} x", "x {\"a\":1}", "{\"a\":1}}", "{\"a\":1}{\"b\":2}",
                            "{\"a\":\"x}", "[1,2]", "\"s\"", "12", "{\"a\":1,\"b\"}", "{a:1}", "{\"a\"\"b\":1}", "{\"a\":1 \"b\":2}", "{\"a\",1}",
                            "{ x }", "{\"a\":1]", "}{"})
        CHECK(!well_formed(bad));
    CHECK(!well_formed("{\"a" + BS + "x\":1}"));  // a key is a string token: its escapes too
    CHECK(jl::record_fields(2) == 0 && jl::record_fields(3) == 1 && jl::record_fields(11) == 5);
}

static void test_host_pieces() {
    uint8_t byte = 0;
    void* out = nullptr;
    uint64_t stats[8];
    CHECK(jl::open_error(&byte, 1, 10000, 0, &out, stats).empty());
    CHECK(jl::open_error(nullptr, 1ull << 32, 0, 1, nullptr, nullptr).find("infer_rows") != std::string::npos);
    CHECK(jl::open_error(nullptr, 1ull << 32, 1, 1, nullptr, nullptr) == "unknown flags");
    CHECK(jl::open_error(nullptr, 1ull << 32, 1, 0, nullptr, nullptr).find("2^32") != std::string::npos);
    CHECK(jl::open_error(nullptr, 5, 1, 0, nullptr, nullptr) == "bytes is NULL");
    CHECK(jl::open_error(&byte, 5, 1, 0, nullptr, nullptr) == "out is NULL");
    CHECK(jl::open_error(&byte, 5, ~0ull, 0, &out, nullptr) == "stats8 is NULL");
    CHECK(jl::open_error(nullptr, 0, 1, 0, &out, stats).empty());
    jl::Names names;
    const std::string text = "\"b\"\"a" + U + "0062\"\"b\"\"\"\"ab\"";
    const uint32_t lens[5] = {3, 9, 3, 2, 4};
    names.add_keys(lens, 5, (const uint8_t*)text.data());
    CHECK(names.count() == 3 && names.offsets == std::vector<uint64_t>({0, 1, 3, 3}));
    CHECK(std::string(names.bytes.begin(), names.bytes.end()) == "bab");
    const jl::IndexLease a(1), b(1000);
    CHECK(a.total % 256 == 0 && b.total > a.total && b.depth_in % 8 == 0 && b.kept_scan % 8 == 0 && b.rec_sums + (oxh::csv::scan_tiles_of(1000) + 1) * 8 <= b.total);
    const jl::SchemaLease s(10000);
    CHECK(s.total % 256 == 0 && s.bytes_scan + 10000 * 8 <= s.sums && s.mask % 8 == 0);
}

int main() {
    test_grammar();
    test_unescape();
    test_carries();
    test_records();
    test_host_pieces();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
