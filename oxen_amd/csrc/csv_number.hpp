// oxen_amd/csrc/csv_number.hpp -- the text of one CSV cell as a typed value (oxh_csv_*, csv_read.hip): the
// grammars of include/oxen_hash.h "CSV", the int64 parse with its overflow check, the float digit accumulation
// with the test for the exact path, the bool match, the quotes of a field and the class bits the inference ANDs.
// Plain C++ that both sides compile (`__host__ __device__` under hipcc, nothing under g++), as sort_keys.hpp is:
// the kernels and tests/native/csv_host_test.cpp run the same code. Every function reads its bytes once, in
// order, through the pointer it is given: no per-lane array, no table (the powers of ten are the caller's).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OXH_CSV_HD __host__ __device__ __forceinline__
#else
#define OXH_CSV_HD inline
#endif

namespace oxh::csvnum {

constexpr uint32_t kNoQuote = 256;  // OXH_CSV_NO_QUOTE: no byte is a quote
// class bits of one cell (the inference ANDs them per column): the text is an INT64 in range / matches the
// FLOAT64 grammar / is a BOOL. An empty cell has all of them.
constexpr uint32_t kIntOk = 1, kFloatOk = 2, kBoolOk = 4, kAllOk = 7;
// parse_int64
constexpr uint32_t kIntNoMatch = 0, kIntValue = 1, kIntOutOfRange = 2;
// parse_float
constexpr uint32_t kFloatNoMatch = 0;   // not the grammar
constexpr uint32_t kFloatExact = 1;     // (-1)^neg * m * 10^e10 is one IEEE operation: m <= 2^53 and |e10| <= 22 (or m == 0)
constexpr uint32_t kFloatDeferred = 2;  // the grammar, but not the exact path: the host converts the text
constexpr uint32_t kFloatInf = 3, kFloatNan = 4;
constexpr int32_t kExactPow10 = 22;     // 10^22 is the largest power of ten a double holds exactly
constexpr uint64_t kExactMantissa = 1ull << 53;
constexpr uint32_t kMaxDigits = 19;     // significant digits a u64 always holds
constexpr uint64_t kQuietNan = 0x7FF8000000000000ull, kInfBits = 0x7FF0000000000000ull, kSignBit = 0x8000000000000000ull;

OXH_CSV_HD bool is_digit(uint32_t c) { return c - '0' < 10u; }
OXH_CSV_HD uint32_t lower(uint32_t c) { return c | 0x20; }  // of an ASCII letter

// The value of a field: one whose first and last bytes are both the quote (length >= 2) loses them. Doubled
// quotes inside are still doubled in [p, p + n): only a string column's copy halves them, and no number or
// boolean holds a quote.
OXH_CSV_HD bool strip_quotes(const uint8_t*& p, uint32_t& n, uint32_t quote) {
    if (quote >= kNoQuote || n < 2 || p[0] != quote || p[n - 1] != quote) return false;
    p += 1, n -= 2;
    return true;
}

// [+-]?[0-9]+ , exact. kIntOutOfRange: the grammar, but not an int64 (a null, never a wrapped value).
OXH_CSV_HD uint32_t parse_int64(const uint8_t* p, uint32_t n, int64_t& out) {
    uint32_t i = 0;
    bool neg = false;
    if (n && (p[0] == '+' || p[0] == '-')) neg = p[0] == '-', i = 1;
    if (i == n) return kIntNoMatch;
    const uint64_t limit = neg ? 1ull << 63 : (1ull << 63) - 1;
    uint64_t acc = 0;
    bool over = false;
    for (; i < n; ++i) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d >= 10u) return kIntNoMatch;
        if (acc > (limit - d) / 10) over = true;  // acc * 10 + d > limit; sticky, the digits are still checked
        acc = acc * 10 + d;
    }
    if (over) return kIntOutOfRange;
    out = neg ? (int64_t)(0 - acc) : (int64_t)acc;
    return kIntValue;
}

// true / false, ASCII case-insensitive.
OXH_CSV_HD bool parse_bool(const uint8_t* p, uint32_t n, bool& out) {
    if (n == 4 && lower(p[0]) == 't' && lower(p[1]) == 'r' && lower(p[2]) == 'u' && lower(p[3]) == 'e') {
        out = true;
        return true;
    }
    if (n == 5 && lower(p[0]) == 'f' && lower(p[1]) == 'a' && lower(p[2]) == 'l' && lower(p[3]) == 's' && lower(p[4]) == 'e') {
        out = false;
        return true;
    }
    return false;
}

// m * 10^e10 (or m / 10^-e10) is one correctly rounded operation on two exact doubles.
OXH_CSV_HD bool exact_path(uint64_t m, int32_t e10) { return m <= kExactMantissa && e10 >= -kExactPow10 && e10 <= kExactPow10; }

// [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?  or  [+-]?(inf|infinity|nan), case-insensitive.
// Up to kMaxDigits significant digits go into m (leading zeros are none), every further one makes the cell
// kFloatDeferred; e10 is the decimal exponent of m's last digit. An exponent beyond +-100000 is clamped there
// (far outside the exact path, and the host reads the text itself).
OXH_CSV_HD uint32_t parse_float(const uint8_t* p, uint32_t n, uint64_t& m, int32_t& e10, bool& neg) {
    uint32_t i = 0;
    neg = false, m = 0, e10 = 0;
    if (n && (p[0] == '+' || p[0] == '-')) neg = p[0] == '-', i = 1;
    const uint32_t rest = n - i;
    if (rest == 3) {
        const uint32_t a = lower(p[i]), b = lower(p[i + 1]), c = lower(p[i + 2]);
        if (a == 'i' && b == 'n' && c == 'f') return kFloatInf;
        if (a == 'n' && b == 'a' && c == 'n') return kFloatNan;
    }
    if (rest == 8) {
        const uint64_t word = 0x7974696E69666E69ull;  // "infinity", first letter in the low byte
        bool same = true;
        for (uint32_t k = 0; k < 8; ++k) same = same && lower(p[i + k]) == ((word >> (8 * k)) & 0xFF);
        if (same) return kFloatInf;
    }
    uint32_t sig = 0, digits = 0;
    bool more = false;  // a significant digit past kMaxDigits
    for (; i < n && is_digit(p[i]); ++i, ++digits) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (m == 0 && d == 0) continue;
        if (sig < kMaxDigits)
            m = m * 10 + d, ++sig;
        else
            more = true, ++e10;
    }
    if (i < n && p[i] == '.') {
        for (++i; i < n && is_digit(p[i]); ++i, ++digits) {
            const uint32_t d = (uint32_t)p[i] - '0';
            if (m == 0 && d == 0) {
                --e10;
                continue;
            }
            if (sig < kMaxDigits)
                m = m * 10 + d, ++sig, --e10;
            else
                more = true;
        }
    }
    if (!digits) return kFloatNoMatch;
    if (i < n && lower(p[i]) == 'e') {
        ++i;
        bool eneg = false;
        if (i < n && (p[i] == '+' || p[i] == '-')) eneg = p[i] == '-', ++i;
        if (i == n) return kFloatNoMatch;
        int32_t x = 0;
        for (; i < n; ++i) {
            if (!is_digit(p[i])) return kFloatNoMatch;
            if (x < 100000) x = x * 10 + (int32_t)(p[i] - '0');
        }
        if (x > 100000) x = 100000;
        e10 += eneg ? -x : x;
    }
    if (i != n) return kFloatNoMatch;
    if (m == 0 && !more) return kFloatExact;  // a zero, whatever its exponent
    if (more) return kFloatDeferred;
    return exact_path(m, e10) ? kFloatExact : kFloatDeferred;
}

// The exact path's value; pow10 = the caller's table of 10^0 .. 10^22 (constant memory on the device). Plain * and /.
OXH_CSV_HD double exact_value(uint64_t m, int32_t e10, bool neg, const double* pow10) {
    if (m == 0) return neg ? -0.0 : 0.0;  // whatever the exponent: it may lie far outside the table
    const double x = (double)m;
    const double v =e10 < 0 ? x / pow10[-e10] : x * pow10[e10];
    return neg ? -v : v;
}

// The class bits of a cell's value (after strip_quotes): what the inference ANDs over a column's cells.
OXH_CSV_HD uint32_t class_bits(const uint8_t* p, uint32_t n) {
    if (n == 0) return kAllOk;
    int64_t iv;
    uint64_t m;
    int32_t e;
    bool neg, bv;
    return (parse_int64(p, n, iv) == kIntValue ? kIntOk : 0) | (parse_float(p, n, m, e, neg) != kFloatNoMatch ? kFloatOk : 0) |
           (parse_bool(p, n, bv) ? kBoolOk : 0);
}

}  // namespace oxh::csvnum
