// oxen_amd/csrc/csv_text.hpp -- a typed value as the text of one CSV cell (oxh_write_csv_*, csv_write.hip): the rules
// of include/oxen_hash.h "CSV text" -- the integer text, the digits-and-exponent of a double to ryu's form, the exact
// path that finds those digits where one IEEE division proves them, and the "necessary" quoting of a string. Plain
// C++ that both sides compile (`__host__ __device__` under hipcc, nothing under g++), as csv_number.hpp is: the
// kernels, the host's deferral and tests/native/csv_write_host_test.cpp run the same code. Every function writes
// through the pointer it is given, in order, or only measures when that pointer is NULL: no per-lane array, no table
// (the powers of ten are the caller's). The last part, the host's conversion of a deferred double, is host code.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <charconv>

#if defined(__HIPCC__)
#define OXH_TEXT_HD __host__ __device__ __forceinline__
#else
#define OXH_TEXT_HD inline
#endif

namespace oxh::csvtext {

constexpr uint32_t kLongCell = 512;     // a string cell of this many bytes and more is a whole wave's
constexpr uint32_t kMaxFloatText = 24;  // -2.2250738585072014e-308
constexpr uint32_t kDeferSlot = 32;     // a deferred double's text, its length in the slot's last byte
constexpr int32_t kExactPow10 = 22;     // 10^22 is the largest power of ten a double holds exactly
constexpr double kExactBelow = 1e15;    // the exact path's digits are an integer below this
constexpr double kMinNormal = 2.2250738585072014e-308;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull, kSignBit = 0x8000000000000000ull;
// what a double is to the writer
constexpr uint32_t kFormZero = 0, kFormNan = 1, kFormInf = 2, kFormDigits = 3, kFormDeferred = 4;

// How many decimal digits v has (1 .. 20).
OXH_TEXT_HD uint32_t digits_u64(uint64_t v) {
    uint32_t n = 1;
    for (uint64_t p = 10; n < 20 && v >= p; p *= 10) ++n;
    return n;
}

OXH_TEXT_HD uint64_t pow10_u64(uint32_t n) {  // n <= 19
    uint64_t p = 1;
    for (uint32_t i = 0; i < n; ++i) p *= 10;
    return p;
}

// The n decimal digits of v (v < 10^n, leading zeros kept) at dst[0 .. n).
OXH_TEXT_HD void put_digits(uint8_t* dst, uint64_t v, uint32_t n) {
    for (uint32_t i = n; i-- > 0;) {
        dst[i] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
}

// OXH_CSV_INT64: decimal digits, '-' in front of a negative. Returns the length (1 .. 20); dst NULL: only that.
OXH_TEXT_HD uint32_t int64_text(int64_t x, uint8_t* dst) {
    const bool neg = x < 0;
    const uint64_t mag = neg ? 0 - (uint64_t)x : (uint64_t)x;
    const uint32_t n = digits_u64(mag);
    if (dst) {
        if (neg) *dst++ = '-';
        put_digits(dst, mag, n);
    }
    return n + (neg ? 1 : 0);
}

// A double as the writer sees it: one of the three words, or the shortest digits d (L of them, no trailing zero) with
// value = d * 10^k, or deferred to the host.
struct FloatForm {
    uint64_t d;
    uint32_t L;
    int32_t k;
    uint32_t kind;
    bool neg;
};

// The exact path: the shortest digits of a finite a > 0, where they are an integer m < 10^15 with a = m / 10^j for a
// j in 0 .. 22. t = a * 10^j is only a guess at m; the test is the division: m and 10^j are both exact doubles, so
// double(m) / 10^j is the correctly rounded value of the decimal m * 10^-j, and equality says that this decimal
// reads back as a. At most one decimal of 15 digits or fewer lies in a double's rounding interval, so the first j
// that passes gives the shortest digits (m without its trailing zeros). false: not proven here -- subnormals, a >=
// 10^15, doubles whose shortest digits are 16 or 17 long, digits further than 22 places behind the point.
// pow10: 1e0 .. 1e22. Needs IEEE division and round-to-nearest-even (no fast-math).
OXH_TEXT_HD bool exact_digits(double a, const double* pow10, uint64_t& d, uint32_t& L, int32_t& k) {
    if (!(a >= kMinNormal) || !(a < kExactBelow)) return false;
    for (int32_t j = 0; j <= kExactPow10; ++j) {
        const double t = a * pow10[j];
        if (t >= kExactBelow) return false;
        const double m = nearbyint(t);
        if (m / pow10[j] == a) {
            uint64_t digits = (uint64_t)m;  // > 0: 0 / 10^j is not a
            int32_t e = -j;
            while (digits % 10 == 0) digits /= 10, ++e;
            d = digits, L = digits_u64(digits), k = e;
            return true;
        }
    }
    return false;
}

OXH_TEXT_HD FloatForm float_form(uint64_t bits, const double* pow10) {
    FloatForm f{0, 0, 0, kFormDeferred, (bits & kSignBit) != 0};
    const uint64_t mag = bits & ~kSignBit;
    if (mag > kInfBits) {
        f.kind = kFormNan;
    } else if (mag == kInfBits) {
        f.kind = kFormInf;
    } else if (mag == 0) {
        f.kind = kFormZero;
    } else {
        double a;
        __builtin_memcpy(&a, &mag, 8);
        if (exact_digits(a, pow10, f.d, f.L, f.k)) f.kind = kFormDigits;
    }
    return f;
}

// ryu's Buffer::format of a finite non-zero double from its shortest digits: with kk = L + k (10^(kk-1) <= |x| <
// 10^kk)
//   0 <= k and kk <= 16   digits, k zeros, ".0"         0 < kk <= 16   the point after kk digits
//   -5 < kk <= 0          "0.", -kk zeros, digits       L == 1         d "e" (kk - 1)
//   otherwise             d0 "." rest "e" (kk - 1)      -- no '+' and no zero padding in the exponent.
// Returns the length (at most kMaxFloatText); dst NULL: only that. The one function of the device and of the host's
// deferral.
OXH_TEXT_HD uint32_t digits_text(bool neg, uint64_t d, uint32_t L, int32_t k, uint8_t* dst) {
    uint32_t o = 0;
    const int32_t kk = (int32_t)L + k;
    if (neg) {
        if (dst) dst[o] = '-';
        ++o;
    }
    if (k >= 0 && kk <= 16) {
        if (dst) {
            put_digits(dst + o, d, L);
            for (int32_t z = 0; z < k; ++z) dst[o + L + z] = '0';
            dst[o + kk] = '.', dst[o + kk + 1] = '0';
        }
        return o + (uint32_t)kk + 2;
    }
    if (kk > 0 && kk <= 16) {  // k < 0: the point falls inside the digits
        if (dst) {
            const uint64_t p = pow10_u64(L - (uint32_t)kk);
            put_digits(dst + o, d / p, (uint32_t)kk);
            dst[o + kk] = '.';
            put_digits(dst + o + kk + 1, d % p, L - (uint32_t)kk);
        }
        return o + L + 1;
    }
    if (kk > -5 && kk <= 0) {
        if (dst) {
            dst[o] = '0', dst[o + 1] = '.';
            for (int32_t z = 0; z < -kk; ++z) dst[o + 2 + z] = '0';
            put_digits(dst + o + 2 - kk, d, L);
        }
        return o + 2 + (uint32_t)(-kk) + L;
    }
    if (L == 1) {
        if (dst) dst[o] = (uint8_t)('0' + d);
        o += 1;
    } else {
        if (dst) {
            const uint64_t p = pow10_u64(L - 1);
            dst[o] = (uint8_t)('0' + d / p), dst[o + 1] = '.';
            put_digits(dst + o + 2, d % p, L - 1);
        }
        o += L + 1;
    }
    const int32_t e = kk - 1;
    const uint32_t mag = (uint32_t)(e < 0 ? -e : e), n = digits_u64(mag);
    if (dst) {
        dst[o] = 'e';
        if (e < 0) dst[o + 1] = '-';
        put_digits(dst + o + 1 + (e < 0 ? 1 : 0), mag, n);
    }
    return o + 1 + (e < 0 ? 1 : 0) + n;
}

// OXH_CSV_FLOAT64 of a form that is not deferred: every NaN is "NaN", the infinities "inf" / "-inf", the zeros "0.0"
// / "-0.0", else digits_text.
OXH_TEXT_HD uint32_t form_text(const FloatForm& f, uint8_t* dst) {
    if (f.kind == kFormDigits) return digits_text(f.neg, f.d, f.L, f.k, dst);
    if (f.kind == kFormNan) {
        if (dst) dst[0] = 'N', dst[1] = 'a', dst[2] = 'N';
        return 3;
    }
    const uint32_t o = f.neg ? 1 : 0;
    if (dst) {
        if (f.neg) dst[0] = '-';
        if (f.kind == kFormInf)
            dst[o] = 'i', dst[o + 1] = 'n', dst[o + 2] = 'f';
        else
            dst[o] = '0', dst[o + 1] = '.', dst[o + 2] = '0';
    }
    return o + 3;
}

OXH_TEXT_HD uint32_t bool_text(bool v, uint8_t* dst) {
    if (dst) {
        if (v)
            dst[0] = 't', dst[1] = 'r', dst[2] = 'u', dst[3] = 'e';
        else
            dst[0] = 'f', dst[1] = 'a', dst[2] = 'l', dst[3] = 's', dst[4] = 'e';
    }
    return v ? 4 : 5;
}

// Strings, quote style "necessary": a cell is quoted iff it is empty or holds the separator, the quote, '\n' or '\r'.
OXH_TEXT_HD bool is_hazard(uint32_t c, uint32_t sep, uint32_t quote) { return c == sep || c == quote || c == '\n' || c == '\r'; }

// The length of the n bytes at p as a cell: as they are, or inside quotes with every quote doubled.
OXH_TEXT_HD uint64_t string_text_len(const uint8_t* p, uint64_t n, uint32_t sep, uint32_t quote, bool& quoted) {
    uint64_t quotes = 0;
    bool hazard = n == 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t c = p[i];
        quotes += c == quote;
        hazard |= is_hazard(c, sep, quote);
    }
    quoted = hazard;
    return hazard ? n + quotes + 2 : n;
}

// A quoted cell, byte by byte.
OXH_TEXT_HD void quoted_text_put(const uint8_t* p, uint64_t n, uint32_t quote, uint8_t* dst) {
    uint64_t o = 0;
    dst[o++] = (uint8_t)quote;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t c = p[i];
        dst[o++] = c;
        if (c == quote) dst[o++] = c;
    }
    dst[o] = (uint8_t)quote;
}

// Whether a separator or quote byte can occur in the text of a number or boolean: 0-9 + - . and the ASCII letters.
OXH_TEXT_HD bool in_number_text(uint32_t c) {
    return c - '0' < 10u || c == '+' || c == '-' || c == '.' || (c | 0x20) - 'a' < 26u;
}

// ---------------------------------------------------------------- host only
// The shortest digits of any finite a > 0, by std::to_chars (shortest round trip, scientific): "d[.ddd]e[+-]xx".
inline void shortest_digits_host(double a, uint64_t& d, uint32_t& L, int32_t& k) {
    char buf[40];
    const std::to_chars_result r = std::to_chars(buf, buf + sizeof buf, a, std::chars_format::scientific);
    uint64_t digits = 0;
    int32_t after_first = 0, e = 0;
    const char* p = buf;
    for (; p < r.ptr && *p != 'e'; ++p) {
        if (*p == '.') continue;
        digits = digits * 10 + (uint64_t)(*p - '0');
        ++after_first;
    }
    if (p < r.ptr) {
        ++p;  // 'e'
        const bool neg = *p == '-';
        if (*p == '-' || *p == '+') ++p;
        for (; p < r.ptr; ++p) e = e * 10 + (*p - '0');
        if (neg) e = -e;
    }
    e -= after_first - 1;
    while (digits && digits % 10 == 0) digits /= 10, ++e;
    d = digits, L = digits_u64(digits), k = e;
}

// A deferred cell (a finite non-zero double the exact path did not prove) into its slot: the text, its length in the
// slot's last byte.
inline void deferred_slot(uint64_t bits, uint8_t* slot) {
    const uint64_t mag = bits & ~kSignBit;
    double a;
    memcpy(&a, &mag, 8);
    uint64_t d;
    uint32_t L;
    int32_t k;
    shortest_digits_host(a, d, L, k);
    memset(slot, 0, kDeferSlot);
    slot[kDeferSlot - 1] = (uint8_t)digits_text((bits & kSignBit) != 0, d, L, k, slot);
}

}  // namespace oxh::csvtext
