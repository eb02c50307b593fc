// oxen_amd/csrc/parquet_bits.hpp -- what the Parquet reader's host code and kernels share (parquet_read_host.hpp,
// parquet_read.hip): a bounded span, the varint, a Thrift compact reader that walks and skips fields without
// recursion, the PageHeader, the run header of the RLE / bit-packed hybrid and the extraction of value k of width w
// from a bit-packed run. Every read is bounded by the span it belongs to: a read past the end sets `bad` and gives
// 0, it never touches the byte. Plain C++, __host__ __device__ under hipcc, so that a stand-alone program can call
// it (tests/native/parquet_read_host_test.cpp, which is also what a sanitizer build runs).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OXH_PQR_BOTH __host__ __device__ inline
#else
#define OXH_PQR_BOTH inline
#endif

namespace oxh::pqr {

struct Span {
    const uint8_t* p;
    uint64_t n;   // bytes of the span
    uint64_t at;  // the next byte
    bool bad;     // a read went past the end, or a value was malformed
};

OXH_PQR_BOTH uint32_t byte(Span& s) {
    if (s.at >= s.n) {
        s.bad = true;
        return 0;
    }
    return s.p[s.at++];
}

OXH_PQR_BOTH void skip_bytes(Span& s, uint64_t n) {
    if (n > s.n - s.at)
        s.bad = true, s.at = s.n;
    else
        s.at += n;
}

// ULEB128, at most 10 bytes.
OXH_PQR_BOTH uint64_t varint(Span& s) {
    uint64_t v = 0;
    for (uint32_t shift = 0; shift < 70; shift += 7) {
        const uint32_t b = byte(s);
        if (s.bad) return 0;
        if (shift < 64) v |= (uint64_t)(b & 0x7F) << shift;
        if (!(b & 0x80)) return v;
    }
    s.bad = true;
    return 0;
}

OXH_PQR_BOTH int64_t zigzag(uint64_t v) { return (int64_t)(v >> 1) ^ -(int64_t)(v & 1); }
OXH_PQR_BOTH int64_t zint(Span& s) { return zigzag(varint(s)); }

OXH_PQR_BOTH uint32_t le32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ---------------------------------------------------------------- Thrift compact protocol
enum : uint32_t { kTStop = 0, kTTrue = 1, kTFalse = 2, kTByte = 3, kTI16 = 4, kTI32 = 5, kTI64 = 6, kTDouble = 7, kTBinary = 8, kTList = 9,
                  kTSet = 10, kTMap = 11, kTStruct = 12 };
constexpr int kSkipDepth = 16;

// The next field of the struct the span stands in: false at its stop byte (consumed) or on a bad span. last: the
// struct's previous field id (0 at its start). A boolean field's value is its type.
OXH_PQR_BOTH bool next_field(Span& s, int32_t& last, int32_t& id, uint32_t& type) {
    const uint32_t b = byte(s);
    if (s.bad || b == 0) return false;
    type = b & 15;
    const uint32_t delta = b >> 4;
    id = delta ? last + (int32_t)delta : (int32_t)zint(s);
    last = id;
    return !s.bad;
}

// A list's header: its element type and count.
OXH_PQR_BOTH void list_header(Span& s, uint32_t& elem, uint64_t& count) {
    const uint32_t h = byte(s);
    elem = h & 15, count = h >> 4;
    if (count == 15) count = varint(s);
}

// Skips one value of `type`, whatever it holds, without recursion (a kernel calls it). st: kSkipDepth words of the
// caller's for the open containers -- a local array on the host, a lane's slice of LDS in a kernel, so that a kernel
// needs no scratch memory. A word is the element type << 56 | the elements left; type kTStop: the fields of a struct.
// A map (the format's metadata has none) and nesting deeper than kSkipDepth make the span bad.
OXH_PQR_BOTH void skip_value(Span& s, uint32_t type, uint64_t* st) {
    constexpr uint64_t kLeft = (1ull << 56) - 1;
    if (type == kTStop) {  // no field has the stop's type
        s.bad = true;
        return;
    }
    int d = 1;
    st[0] = (uint64_t)type << 56 | 1;
    while (d > 0 && !s.bad) {
        const uint32_t elem = (uint32_t)(st[d - 1] >> 56);
        uint32_t t;
        if (elem == kTStop) {
            const uint32_t b = byte(s);
            if (s.bad || b == 0) {
                --d;
                continue;
            }
            t = b & 15;
            if ((b >> 4) == 0) (void)varint(s);
            if (t == kTTrue || t == kTFalse) continue;
        } else {
            if ((st[d - 1] & kLeft) == 0) {
                --d;
                continue;
            }
            --st[d - 1];
            t = elem;
            if (t == kTTrue || t == kTFalse) {  // a list's booleans are a byte each
                (void)byte(s);
                continue;
            }
        }
        switch (t) {
            case kTByte: (void)byte(s); break;
            case kTI16:
            case kTI32:
            case kTI64: (void)varint(s); break;
            case kTDouble: skip_bytes(s, 8); break;
            case kTBinary: {
                const uint64_t n = varint(s);
                skip_bytes(s, n);
                break;
            }
            case kTList:
            case kTSet: {
                uint32_t e;
                uint64_t count;
                list_header(s, e, count);
                if (count > s.n - s.at) count = s.n - s.at + 1;  // every element takes a byte: the span ends first
                if (d == kSkipDepth || e == kTStop) {
                    s.bad = true;
                    break;
                }
                st[d++] = (uint64_t)e << 56 | count;
                break;
            }
            case kTStruct:
                if (d == kSkipDepth) {
                    s.bad = true;
                    break;
                }
                st[d++] = (uint64_t)kTStop << 56;
                break;
            default: s.bad = true; break;
        }
    }
}

// ---------------------------------------------------------------- PageHeader
enum : int32_t { kPageData = 0, kPageIndex = 1, kPageDict = 2, kPageDataV2 = 3 };
enum : int32_t { kEncPlain = 0, kEncPlainDict = 2, kEncRle = 3, kEncBitPacked = 4, kEncRleDict = 8 };

struct PageInfo {
    int32_t type, usize, csize;        // PageHeader 1, 2, 3
    int32_t num_values, encoding;      // of the page's own header struct
    int32_t def_enc, rep_enc;          // V1
    int32_t def_len, rep_len;          // V2: the levels' bytes
    uint32_t is_compressed;            // V2 (default true)
    uint32_t has;                      // bit 0: a V1 struct, 1: a dictionary struct, 2: a V2 struct
};

OXH_PQR_BOTH int32_t i32_field(Span& s) {
    const int64_t v = zint(s);
    if (v < INT32_MIN || v > INT32_MAX) s.bad = true;
    return (int32_t)v;
}

// The PageHeader the span starts with; s.at is then the first byte of the page's body. false: the span is bad. st:
// skip_value's words.
OXH_PQR_BOTH bool page_header(Span& s, PageInfo& h, uint64_t* st) {
    h.type = -1, h.usize = h.csize = -1, h.num_values = -1, h.encoding = -1, h.def_enc = h.rep_enc = -1, h.def_len = h.rep_len = 0;
    h.is_compressed = 1, h.has = 0;
    int32_t last = 0, id;
    uint32_t type;
    while (next_field(s, last, id, type)) {
        if (id == 1 && type == kTI32) {
            h.type = i32_field(s);
        } else if (id == 2 && type == kTI32) {
            h.usize = i32_field(s);
        } else if (id == 3 && type == kTI32) {
            h.csize = i32_field(s);
        } else if ((id == 5 || id == 7 || id == 8) && type == kTStruct) {
            h.has |= id == 5 ? 1u : id == 7 ? 2u : 4u;
            int32_t l2 = 0, i2;
            uint32_t t2;
            while (next_field(s, l2, i2, t2)) {
                const bool word = t2 == kTI32;
                if (word && i2 == 1) {
                    h.num_values = i32_field(s);
                } else if (word && i2 == 2 && id != 8) {
                    h.encoding = i32_field(s);
                } else if (word && id == 5 && i2 == 3) {
                    h.def_enc = i32_field(s);
                } else if (word && id == 5 && i2 == 4) {
                    h.rep_enc = i32_field(s);
                } else if (word && id == 8 && i2 == 4) {
                    h.encoding = i32_field(s);
                } else if (word && id == 8 && i2 == 5) {
                    h.def_len = i32_field(s);
                } else if (word && id == 8 && i2 == 6) {
                    h.rep_len = i32_field(s);
                } else if (id == 8 && i2 == 7 && (t2 == kTTrue || t2 == kTFalse)) {
                    h.is_compressed = t2 == kTTrue;
                } else if (t2 != kTTrue && t2 != kTFalse) {
                    skip_value(s, t2, st);
                }
            }
        } else if (type != kTTrue && type != kTFalse) {
            skip_value(s, type, st);
        }
    }
    return !s.bad;
}

// ---------------------------------------------------------------- the RLE / bit-packed hybrid
constexpr uint64_t kMaxGroups = 1ull << 40;  // a run header beyond any page: clamped, so that no product overflows

// A run's header: `count` values, bit-packed (8 per group) or one repeated value. false: the span is bad or the run
// is empty (a walk over empty runs would never end).
OXH_PQR_BOTH bool run_header(Span& s, uint64_t& count, bool& packed) {
    const uint64_t h = varint(s);
    packed = h & 1;
    uint64_t n = h >> 1;
    if (n > kMaxGroups) n = kMaxGroups;
    count = packed ? n * 8 : n;
    return !s.bad && count != 0;
}

// A repeated run's value: ceil(w / 8) bytes, little-endian; it must fit w bits.
OXH_PQR_BOTH uint32_t run_value(Span& s, uint32_t w) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < (w + 7) / 8; ++b) v |= byte(s) << (8 * b);
    if (w < 32 && (v >> w)) s.bad = true;
    return v;
}

// Value k of width w (0 .. 32) of the bit-packed run whose `avail` bytes start at p. Bytes past avail read as 0.
OXH_PQR_BOTH uint32_t extract(const uint8_t* p, uint64_t avail, uint64_t k, uint32_t w) {
    if (!w) return 0;
    const uint64_t bit = k * w, first = bit >> 3;
    const uint32_t sh = (uint32_t)(bit & 7), nb = (sh + w + 7) / 8;  // at most 5 bytes
    uint64_t v = 0;
    for (uint32_t b = 0; b < nb; ++b)
        if (first + b < avail) v |= (uint64_t)p[first + b] << (8 * b);
    return (uint32_t)(v >> sh) & (w == 32 ? 0xFFFFFFFFu : (1u << w) - 1);
}

// One run of a hybrid stream, ready to be read: value j < count is `value` (RLE) or extract(body, avail, j, w).
struct Run {
    uint64_t count;
    const uint8_t* body;
    uint64_t avail;
    uint32_t value;
    bool packed;
};

// The next run of the stream; `want` values are still missing (a writer may cut the last group's bytes short, so
// only the bytes of min(count, want) values must be there). false: the stream is malformed or ends early.
OXH_PQR_BOTH bool next_run(Span& s, uint32_t w, uint64_t want, Run& r) {
    if (!run_header(s, r.count, r.packed)) return false;
    r.body = s.p + s.at, r.value = 0, r.avail = 0;
    if (r.packed) {
        const uint64_t full = r.count / 8 * w, left = s.n - s.at;
        r.avail = full < left ? full : left;
        const uint64_t take = r.count < want ? r.count : want;
        if ((take * w + 7) / 8 > r.avail) return s.bad = true, false;
        s.at += r.avail;
    } else {
        r.value = run_value(s, w);
    }
    return !s.bad;
}

}  // namespace oxh::pqr
