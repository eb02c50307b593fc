// oxen_amd/csrc/json_text.hpp -- a typed value as the text of one JSON value (oxh_write_json_*, json_write.hip): the
// rules of include/oxen_hash.h "JSON text". The numbers and booleans are csv_text.hpp's (the integer text, ryu's form
// of a double from its shortest digits, the exact path and the host's deferral); this file adds the string rule --
// the width of a byte (1, 2 or 6), the escaped length of a span, the byte-by-byte put -- and, for the host, the
// constant text in front of a column's value (its key). Plain C++ that both sides compile, as csv_text.hpp is: the
// kernels, the host and tests/native/json_write_host_test.cpp run the same code. Every function writes through the
// pointer it is given, in order: no per-lane array, no table.
#pragma once

#include "csv_text.hpp"

namespace oxh::jsontext {

constexpr uint32_t kNullText = 4;  // null

// How many bytes c takes inside a JSON string: 2 for '"', '\\' and the five short escapes (\b \f \n \r \t), 6 for
// every other byte below 0x20 (\u00XX), else 1 -- 0x7F, '/' and every byte at or above 0x80 are copied as they are.
OXH_TEXT_HD uint32_t byte_width(uint32_t c) {
    if (c >= 0x20) return c == '"' || c == '\\' ? 2 : 1;
    return c == 0x08 || c == 0x09 || c == 0x0A || c == 0x0C || c == 0x0D ? 2 : 6;
}

// The letter behind the backslash of a byte of width 2.
OXH_TEXT_HD uint8_t short_escape(uint32_t c) {
    return c == 0x08 ? 'b' : c == 0x09 ? 't' : c == 0x0A ? 'n' : c == 0x0C ? 'f' : c == 0x0D ? 'r' : (uint8_t)c;
}

OXH_TEXT_HD uint8_t hex_digit(uint32_t v) { return (uint8_t)(v < 10 ? '0' + v : 'a' + (v - 10)); }

// c as it stands inside a JSON string, at dst[0 .. byte_width(c)). Returns the width.
OXH_TEXT_HD uint32_t byte_put(uint32_t c, uint8_t* dst) {
    const uint32_t w = byte_width(c);
    if (w == 1) {
        dst[0] = (uint8_t)c;
    } else if (w == 2) {
        dst[0] = '\\', dst[1] = short_escape(c);
    } else {
        dst[0] = '\\', dst[1] = 'u', dst[2] = '0', dst[3] = '0', dst[4] = hex_digit(c >> 4), dst[5] = hex_digit(c & 15);
    }
    return w;
}

// The n bytes at p inside a JSON string, without the quotes around them: the sum of their widths.
OXH_TEXT_HD uint64_t escaped_len(const uint8_t* p, uint64_t n) {
    uint64_t l = 0;
    for (uint64_t i = 0; i < n; ++i) l += byte_width(p[i]);
    return l;
}

// A string value, byte by byte, into dst[0 .. room): '"', the escaped bytes, '"'. Returns the length, escaped_len + 2;
// a text that does not fit its room stops in front of the first byte that would not, and returns room + 1.
OXH_TEXT_HD uint64_t string_put(const uint8_t* p, uint64_t n, uint8_t* dst, uint64_t room) {
    if (room < 2) return room + 1;
    uint64_t o = 0;
    dst[o++] = '"';
    for (uint64_t i = 0; i < n; ++i) {
        if (o + byte_width(p[i]) + 1 > room) return room + 1;
        o += byte_put(p[i], dst + o);
    }
    dst[o++] = '"';
    return o;
}

OXH_TEXT_HD void null_put(uint8_t* dst) { dst[0] = 'n', dst[1] = 'u', dst[2] = 'l', dst[3] = 'l'; }

// OXH_CSV_FLOAT64 of a form that is not deferred: every NaN and both infinities are null, else csv_text.hpp's
// form_text (0.0 / -0.0, digits_text). Returns the length; dst NULL: only that.
OXH_TEXT_HD uint32_t float_form_text(const csvtext::FloatForm& f, uint8_t* dst) {
    if (f.kind == csvtext::kFormNan || f.kind == csvtext::kFormInf) {
        if (dst) null_put(dst);
        return kNullText;
    }
    return csvtext::form_text(f, dst);
}

// ---------------------------------------------------------------- host only
// The constant bytes in front of a column's value, appended to `text`: '{' for the first column of a row and ','
// for the others, the name by the string rule, ':' (Bytes: a std::vector<uint8_t>). Returns whether a byte of the name was escaped.
template <class Bytes>
inline bool key_text(const uint8_t* name, uint64_t n, bool first, Bytes& text) {
    text.push_back(first ? '{' : ',');
    const uint64_t l = escaped_len(name, n) + 2;
    const size_t at = text.size();
    text.resize(at + l);
    string_put(name, n, text.data() + at, l);
    text.push_back(':');
    return l != n + 2;
}

}  // namespace oxh::jsontext
