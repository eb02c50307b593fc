// oxen_amd/csrc/jsonl_text.hpp -- the text of JSON Lines as the reader sees it (oxh_jsonl_*, jsonl_read.hip): the
// cell grammar of include/oxen_hash.h "JSON Lines" (string token, nested value, true / false / null, number), the
// unescape step of a string token (one escape, a surrogate pair being one, to 1-4 bytes of UTF-8), the key compare
// through that same step, and the three carries of the index -- "an odd run of backslashes ends here", and the
// string parity and the depth since the last '\n' -- as values with an associative compose, so that a lane, a
// wave, a tile and the whole buffer combine them alike. Plain C++ that both sides compile, as csv_number.hpp is:
// the kernels and tests/native/jsonl_host_test.cpp run the same code.
#pragma once

#include <stdint.h>

#include "csv_number.hpp"

namespace oxh::jsonl {

// the kind of one trimmed value slot
constexpr uint32_t kUnparsable = 0, kString = 1, kNested = 2, kTrue = 3, kFalse = 4, kNull = 5;
constexpr uint32_t kInteger = 6;  // a number token without fraction or exponent
constexpr uint32_t kNumber = 7;   // any other number token

OXH_CSV_HD bool is_ws(uint32_t c) { return c == 0x20 || c == 0x09 || c == 0x0D; }  // '\n' never lies inside a record

// [p, p + n) without the JSON whitespace at both ends.
OXH_CSV_HD void trim(const uint8_t*& p, uint32_t& n) {
    while (n && is_ws(p[0])) ++p, --n;
    while (n && is_ws(p[n - 1])) --n;
}

OXH_CSV_HD int32_t hex4(const uint8_t* p) {
    int32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = p[k];
        uint32_t d;
        if (c - '0' < 10u)
            d = c - '0';
        else if ((c | 0x20) - 'a' < 6u)
            d = (c | 0x20) - 'a' + 10;
        else
            return -1;
        v = v * 16 + (int32_t)d;
    }
    return v;
}

// One escape at p[0] == '\\' with n bytes of the token's interior left: its w bytes (1-4) into out, and how many
// bytes of text it took (2, 6, or 12 for a surrogate pair); 0: not an escape of the grammar (a lone surrogate of
// either kind included).
OXH_CSV_HD uint32_t decode_escape(const uint8_t* p, uint32_t n, uint8_t* out, uint32_t& w) {
    if (n < 2) return 0;
    w = 1;
    switch (p[1]) {
        case '"': out[0] = '"'; return 2;
        case '\\': out[0] = '\\'; return 2;
        case '/': out[0] = '/'; return 2;
        case 'b': out[0] = 8; return 2;
        case 'f': out[0] = 12; return 2;
        case 'n': out[0] = 10; return 2;
        case 'r': out[0] = 13; return 2;
        case 't': out[0] = 9; return 2;
        case 'u': break;
        default: return 0;
    }
    if (n < 6) return 0;
    int32_t cp = hex4(p + 2);
    if (cp < 0 || (cp >= 0xDC00 && cp <= 0xDFFF)) return 0;
    uint32_t took = 6;
    if (cp >= 0xD800 && cp <= 0xDBFF) {
        if (n < 12 || p[6] != '\\' || p[7] != 'u') return 0;
        const int32_t low = hex4(p + 8);
        if (low < 0xDC00 || low > 0xDFFF) return 0;
        cp = 0x10000 + ((cp - 0xD800) << 10) + (low - 0xDC00);
        took = 12;
    }
    if (cp < 0x80) {
        out[0] = (uint8_t)cp;
    } else if (cp < 0x800) {
        out[0] = (uint8_t)(0xC0 | (cp >> 6)), out[1] = (uint8_t)(0x80 | (cp & 0x3F)), w = 2;
    } else if (cp < 0x10000) {
        out[0] = (uint8_t)(0xE0 | (cp >> 12)), out[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)), out[2] = (uint8_t)(0x80 | (cp & 0x3F)), w = 3;
    } else {
        out[0] = (uint8_t)(0xF0 | (cp >> 18)), out[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F)), out[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)),
        out[3] = (uint8_t)(0x80 | (cp & 0x3F)), w = 4;
    }
    return took;
}

// What a walk over a string token does with the unescaped bytes.
struct CountSink {
    uint32_t n = 0;
    OXH_CSV_HD bool put(uint8_t) {
        ++n;
        return true;
    }
};
struct CopySink {
    uint8_t* dst;
    uint32_t n = 0, cap;
    OXH_CSV_HD bool put(uint8_t c) {
        if (n < cap) dst[n] = c;  // never a store past the measured bytes
        ++n;
        return true;
    }
};
struct EqualSink {
    const uint8_t* name;
    uint32_t len, n = 0;
    OXH_CSV_HD bool put(uint8_t c) {
        if (n >= len || name[n] != c) return false;
        ++n;
        return true;
    }
};

// The string token [p, p + n): '"', the interior, an unescaped '"' as its last byte and no other unescaped '"',
// every escape one of the grammar, no raw byte below 0x20. Its unescaped bytes go to the sink in order; false: not
// a string token (or the sink said stop).
template <class Sink>
OXH_CSV_HD bool walk_string(const uint8_t* p, uint32_t n, Sink& sink) {
    if (n < 2 || p[0] != '"' || p[n - 1] != '"') return false;
    const uint32_t end = n - 1;
    for (uint32_t i = 1; i < end;) {
        const uint32_t c = p[i];
        if (c == '"' || c < 0x20) return false;
        if (c == '\\') {
            uint8_t out[4];
            uint32_t w = 0;
            const uint32_t took = decode_escape(p + i, end - i, out, w);
            if (!took) return false;
            for (uint32_t k = 0; k < w; ++k)
                if (!sink.put(out[k])) return false;
            i += took;
        } else {
            if (!sink.put((uint8_t)c)) return false;
            ++i;
        }
    }
    return true;
}

// The unescaped length of a string token; false: not one.
OXH_CSV_HD bool string_token(const uint8_t* p, uint32_t n, uint32_t& out_len) {
    CountSink s;
    if (!walk_string(p, n, s)) return false;
    out_len = s.n;
    return true;
}

// A (valid) string token's unescaped bytes to dst, `cap` of them at most.
OXH_CSV_HD uint32_t unescape_copy(const uint8_t* p, uint32_t n, uint8_t* dst, uint32_t cap) {
    CopySink s{dst, 0, cap};
    (void)walk_string(p, n, s);
    return s.n;
}

// The string token's unescaped text is exactly name[0 .. len).
OXH_CSV_HD bool key_equals(const uint8_t* p, uint32_t n, const uint8_t* name, uint32_t len) {
    EqualSink s{name, len, 0};
    return walk_string(p, n, s) && s.n == len;
}

// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? over the whole of [p, p + n): kInteger, kNumber or kUnparsable.
OXH_CSV_HD uint32_t number_token(const uint8_t* p, uint32_t n) {
    uint32_t i = 0, kind = kInteger;
    if (i < n && p[i] == '-') ++i;
    if (i == n) return kUnparsable;
    if (p[i] == '0') {
        ++i;
    } else if ((uint32_t)p[i] - '1' < 9u) {
        while (i < n && csvnum::is_digit(p[i])) ++i;
    } else {
        return kUnparsable;
    }
    if (i < n && p[i] == '.') {
        ++i;
        if (i == n || !csvnum::is_digit(p[i])) return kUnparsable;
        while (i < n && csvnum::is_digit(p[i])) ++i;
        kind = kNumber;
    }
    if (i < n && (p[i] | 0x20) == 'e') {
        ++i;
        if (i < n && (p[i] == '+' || p[i] == '-')) ++i;
        if (i == n || !csvnum::is_digit(p[i])) return kUnparsable;
        while (i < n && csvnum::is_digit(p[i])) ++i;
        kind = kNumber;
    }
    return i == n ? kind : kUnparsable;
}

OXH_CSV_HD bool is_word(const uint8_t* p, uint32_t n, const char* word, uint32_t len) {
    if (n != len) return false;
    for (uint32_t k = 0; k < len; ++k)
        if (p[k] != (uint8_t)word[k]) return false;
    return true;
}

// The kind of a trimmed, non-empty value slot. A string token is walked whole; str_len = its unescaped bytes.
OXH_CSV_HD uint32_t cell_kind(const uint8_t* p, uint32_t n, uint32_t& str_len) {
    str_len = 0;
    if (!n) return kUnparsable;
    const uint32_t c = p[0];
    if (c == '"') return string_token(p, n, str_len) ? kString : kUnparsable;
    if (c == '{') return p[n - 1] == '}' && n >= 2 ? kNested : kUnparsable;
    if (c == '[') return p[n - 1] == ']' && n >= 2 ? kNested : kUnparsable;
    if (c == 't') return is_word(p, n, "true", 4) ? kTrue : kUnparsable;
    if (c == 'f') return is_word(p, n, "false", 5) ? kFalse : kUnparsable;
    if (c == 'n') return is_word(p, n, "null", 4) ? kNull : kUnparsable;
    if (c == '-' || csvnum::is_digit(c)) return number_token(p, n);
    return kUnparsable;
}

// The kind without the walk over a string's interior: what the class bits and the non-string types need.
OXH_CSV_HD uint32_t cell_kind_shallow(const uint8_t* p, uint32_t n) {
    if (n && p[0] == '"') return kString;
    uint32_t unused;
    return cell_kind(p, n, unused);
}

// The class bits of a cell for the inference (csv_number.hpp's): a null has all, an integer in the int64 range is
// an int and a float, any other number a float, a bool a bool, everything else none.
OXH_CSV_HD uint32_t class_bits(const uint8_t* p, uint32_t n) {
    const uint32_t kind = cell_kind_shallow(p, n);
    if (kind == kNull) return csvnum::kAllOk;
    if (kind == kTrue || kind == kFalse) return csvnum::kBoolOk;
    if (kind == kNumber) return csvnum::kFloatOk;
    if (kind == kInteger) {
        int64_t v;
        return csvnum::parse_int64(p, n, v) == csvnum::kIntValue ? (csvnum::kIntOk | csvnum::kFloatOk) : csvnum::kFloatOk;
    }
    return 0;
}

// ---------------------------------------------------------------- the carries of the index
// bit j of the result: byte j is escaped (the maximal run of backslashes directly before it is odd). bs: the
// backslashes of 16 bytes; carry: an odd run ends directly before byte 0.
OXH_CSV_HD uint32_t escaped_mask(uint32_t bs, uint32_t carry) {
    uint32_t esc = 0, e = carry & 1;
    for (uint32_t j = 0; j < 16; ++j) {
        esc |= e << j;
        e = (bs >> j) & ~e & 1;
    }
    return esc;
}

// "The parity of the run of backslashes that ends with this unit": kEscSet | parity when the unit holds a byte
// that is no backslash, 0 when it is all backslashes -- every such unit (16 bytes, a wave's 1 KiB, a 4 KiB tile)
// has even length and passes what came before through.
constexpr uint32_t kEscSet = 2;
struct EscCarry {
    uint32_t v;
    static OXH_CSV_HD EscCarry identity() { return EscCarry{0}; }
    static OXH_CSV_HD EscCarry compose(EscCarry a, EscCarry b) { return (b.v & kEscSet) ? b : a; }
};
OXH_CSV_HD EscCarry esc_of_lane(uint32_t bs) {
    const uint32_t other = ~bs & 0xFFFF;  // a byte outside the buffer is no backslash
    if (!other) return EscCarry{0};
    const uint32_t top = 31 - (uint32_t)__builtin_clz(other);
    return EscCarry{kEscSet | ((15 - top) & 1)};
}
// The carry into a unit from what its exclusive prefix says, `before` being the carry into the first unit.
OXH_CSV_HD uint32_t esc_in(EscCarry prefix, uint32_t before) { return (prefix.v & kEscSet) ? prefix.v & 1 : before & 1; }

// prefix xor: bit j = the parity of bits 0 .. j
OXH_CSV_HD uint32_t prefix_xor16(uint32_t x) {
    x ^= x << 1, x ^= x << 2, x ^= x << 4, x ^= x << 8;
    return x & 0xFFFF;
}

// What a unit does to (inside a string, depth): without a '\n' it xors `par` and adds d0 or d1 as the unit is
// entered outside or inside a string; with one (`reset`) it leaves (par, d0) whatever came before.
template <class D>
struct LineCarry {
    uint32_t reset, par;
    D d0, d1;
    static OXH_CSV_HD LineCarry identity() { return LineCarry{0, 0, 0, 0}; }
    static OXH_CSV_HD LineCarry compose(LineCarry a, LineCarry b) {
        if (b.reset) return b;
        LineCarry r;
        r.reset = a.reset, r.par = a.par ^ b.par;
        r.d0 = a.d0 + (a.par ? b.d1 : b.d0);
        r.d1 = a.d1 + (a.par ? b.d0 : b.d1);
        return r;
    }
};

// The carry of 16 bytes: uq their unescaped quotes, nl their newlines, op / cl their openers and closers.
OXH_CSV_HD LineCarry<int32_t> line_of_lane(uint32_t uq, uint32_t nl, uint32_t op, uint32_t cl) {
    LineCarry<int32_t> c;
    uint32_t after = 0xFFFF;
    c.reset = nl != 0;
    if (nl) after = 0xFFFF & ~((2u << (31 - (uint32_t)__builtin_clz(nl))) - 1);
    uq &= after, op &= after, cl &= after;
    const uint32_t in = prefix_xor16(uq);
    c.par = (uint32_t)__builtin_popcount(uq) & 1;
    c.d0 = __builtin_popcount(op & ~in) - __builtin_popcount(cl & ~in);
    c.d1 = __builtin_popcount(op & in) - __builtin_popcount(cl & in);
    return c;
}

// The 16 bytes entered with (inside, depth): the bytes the index keeps -- an opener that leaves depth 0, a closer
// that reaches depth 0 or below, a ':' or ',' at depth 1, all outside strings. co: the colons and commas.
OXH_CSV_HD uint32_t kept_of_lane(uint32_t uq, uint32_t nl, uint32_t op, uint32_t cl, uint32_t co, uint32_t inside_in, int64_t depth) {
    uint32_t inside = prefix_xor16(uq) ^ (inside_in ? 0xFFFF : 0);
    for (uint32_t rem = nl; rem;) {  // a line that ends inside a string: the next one starts outside
        const uint32_t k = (uint32_t)__builtin_ctz(rem);
        rem &= rem - 1;
        if ((inside >> k) & 1) inside ^= 0xFFFF & ~((2u << k) - 1);
    }
    uint32_t kept = 0;
    for (uint32_t walk = ((op | cl | co) & ~inside) | nl; walk;) {
        const uint32_t bit = walk & (0 - walk);
        walk &= walk - 1;
        if (nl & bit) {
            depth = 0;
        } else if (op & bit) {
            if (depth == 0) kept |= bit;
            ++depth;
        } else if (cl & bit) {
            if (depth <= 1) kept |= bit;
            --depth;
        } else if (depth == 1) {
            kept |= bit;
        }
    }
    return kept;
}

// ---------------------------------------------------------------- a record over the kept positions
// A line's bytes are [a, b) of `bytes`; s[0 .. m) are its kept positions, ascending. A well-formed record with k
// fields has m = 2 k + 1 of them ("{}" has 2): '{', then ':' and ',' in turn, then '}'.
OXH_CSV_HD bool all_ws(const uint8_t* bytes, uint32_t from, uint32_t to) {
    for (uint32_t i = from; i < to; ++i)
        if (!is_ws(bytes[i])) return false;
    return true;
}

OXH_CSV_HD uint32_t record_fields(uint32_t m) { return m < 3 ? 0 : (m - 1) / 2; }

// The trimmed key / value slot of field f.
OXH_CSV_HD void key_slot(const uint8_t* bytes, const uint32_t* s, uint32_t f, const uint8_t*& p, uint32_t& n) {
    p = bytes + s[2 * f] + 1, n = s[2 * f + 1] - s[2 * f] - 1;
    trim(p, n);
}
OXH_CSV_HD void value_slot(const uint8_t* bytes, const uint32_t* s, uint32_t f, const uint8_t*& p, uint32_t& n) {
    p = bytes + s[2 * f + 1] + 1, n = s[2 * f + 2] - s[2 * f + 1] - 1;
    trim(p, n);
}

OXH_CSV_HD bool record_well_formed(const uint8_t* bytes, uint32_t a, uint32_t b, const uint32_t* s, uint32_t m) {
    if (m < 2 || bytes[s[0]] != '{' || bytes[s[m - 1]] != '}') return false;
    if (!all_ws(bytes, a, s[0]) || !all_ws(bytes, s[m - 1] + 1, b)) return false;
    if (m == 2) return all_ws(bytes, s[0] + 1, s[1]);
    if (!(m & 1)) return false;
    for (uint32_t i = 1; i + 1 < m; ++i)
        if (bytes[s[i]] != ((i & 1) ? ':' : ',')) return false;
    for (uint32_t f = 0; f < record_fields(m); ++f) {
        const uint8_t* p;
        uint32_t n, len;
        key_slot(bytes, s, f, p, n);
        if (!string_token(p, n, len)) return false;
        value_slot(bytes, s, f, p, n);
        if (!n) return false;
    }
    return true;
}

}  // namespace oxh::jsonl
