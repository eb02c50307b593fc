// oxen_amd/csrc/zstd_tables.hpp -- the untrusted arithmetic of a Zstandard block (RFC 8878) with no HIP in it: the
// backward bit reader, an FSE table description to normalised counts to a decode table, Huffman weights (direct or
// FSE-compressed) to a decode table, one Huffman stream's decode, the literals and sequences section headers, the three
// interleaved sequence states and the repeat offsets. The kernel (zstd_inflate.hip) calls these with its tables and work arrays in LDS;
// tests/native/zstd_tables_test.cpp runs them on the CPU, plain and under ASan / UBSan. Every function returns 0 or
// one of the kTab* causes, reads only src[0, n) and writes only inside the arrays whose sizes its comment states.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OXH_ZSTD_BOTH __host__ __device__ inline
#else
#define OXH_ZSTD_BOTH inline
#endif

namespace oxh::zst {

struct FseCell {
    uint16_t base;  // the next state is base + the next nbits bits
    uint8_t symbol, nbits;
};

constexpr uint32_t kMaxLL = 35, kMaxOF = 31, kMaxML = 52;  // the largest code of each kind
constexpr uint32_t kLogLL = 9, kLogOF = 8, kLogML = 9;     // the largest accuracy log of each kind
constexpr uint32_t kLogWeights = 6, kMaxWeight = 11;       // the weights' FSE table; a Huffman code has at most 11 bits
constexpr uint32_t kHufCells = 1u << kMaxWeight;
constexpr uint32_t kFseSymbols = 53;                       // the longest alphabet a table of this file has (ML)

enum : uint32_t {
    kTabOk = 0,
    kTabLog,       // an accuracy log above the kind's maximum
    kTabOverrun,   // a probability larger than what is left of the total
    kTabUnderrun,  // the alphabet ends before the total is reached
    kTabRepeat,    // a zero-repeat run past the alphabet
    kTabInput,     // the description leaves its bytes
    kTabWeights,   // no weights, more than 255, one above 11, or a stream that is not one
    kTabSum,       // the weights' sum is not completable to a power of two of at most 2^11
};

OXH_ZSTD_BOTH uint32_t high_bit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v > 0

// Bits [at, at + count) of the little-endian number src[0, n), count <= 32; bits outside the number are zeros.
OXH_ZSTD_BOTH uint32_t bits_at(const uint8_t* src, uint32_t n, int64_t at, uint32_t count) {
    if (count == 0 || at + (int64_t)count <= 0) return 0;
    const uint32_t lead = at < 0 ? (uint32_t)-at : 0;  // zeros below the number
    const uint64_t from = at < 0 ? 0 : (uint64_t)at;
    const uint64_t byte = from >> 3;
    uint64_t v = 0;
    if (byte + 8 <= n)
        __builtin_memcpy(&v, src + byte, 8);
    else
        for (uint64_t k = byte; k < n; ++k) v |= (uint64_t)src[k] << (8 * (k - byte));
    v >>= from & 7;  // 57 bits and more are left: count - lead <= 32
    const uint32_t take = count - lead;
    return (uint32_t)(v & ((1ull << take) - 1)) << lead;
}

// A stream read from its end: the last byte's highest set bit is the end mark. left: the bits not read yet; it goes
// negative when more was asked for than there is, and the bits that are not there read as zeros.
struct BackBits {
    const uint8_t* src;
    uint32_t n;
    int64_t left;
};
// false: no stream (no byte, or a last byte without the mark).
OXH_ZSTD_BOTH bool back_open(BackBits& b, const uint8_t* src, uint32_t n) {
    b.src = src, b.n = n, b.left = 0;
    if (n == 0 || src[n - 1] == 0) return false;
    b.left = 8 * (int64_t)(n - 1) + high_bit(src[n - 1]);
    return true;
}
OXH_ZSTD_BOTH uint32_t back_read(BackBits& b, uint32_t count) {
    b.left -= count;
    return bits_at(b.src, b.n, b.left, count);
}

// An FSE table description at src[0, n) to norm[0, max_symbol] (-1: "less than 1"; what it does not name is 0),
// *log and *used, the description's whole bytes.
OXH_ZSTD_BOTH uint32_t fse_read_counts(const uint8_t* src, uint32_t n, uint32_t max_log, uint32_t max_symbol, int16_t* norm, uint32_t* log,
                                       uint32_t* used) {
    for (uint32_t s = 0; s <= max_symbol; ++s) norm[s] = 0;
    const uint32_t alog = 5 + bits_at(src, n, 0, 4);
    if (alog > max_log) return kTabLog;
    int32_t remaining = 1 << alog;
    int64_t pos = 4;
    uint32_t sym = 0;
    while (remaining > 0) {
        if (sym > max_symbol) return kTabUnderrun;
        if (pos > 8 * (int64_t)n) return kTabInput;
        const uint32_t nb = high_bit((uint32_t)remaining + 1) + 1;
        uint32_t val = bits_at(src, n, pos, nb);
        const uint32_t low = (1u << (nb - 1)) - 1, threshold = (1u << nb) - 1 - ((uint32_t)remaining + 1);
        if ((val & low) < threshold) {
            val &= low, pos += nb - 1;
        } else {
            if (val > low) val -= threshold;
            pos += nb;
        }
        const int32_t proba = (int32_t)val - 1;
        const int32_t cost = proba < 0 ? 1 : proba;
        if (cost > remaining) return kTabOverrun;
        remaining -= cost;
        norm[sym++] = (int16_t)proba;
        if (proba == 0) {
            uint32_t repeat;
            do {
                if (pos > 8 * (int64_t)n) return kTabInput;
                repeat = bits_at(src, n, pos, 2), pos += 2;
                if (sym + repeat > max_symbol + 1) return kTabRepeat;
                sym += repeat;  // zeros: norm is
            } while (repeat == 3);
        }
    }
    if (pos > 8 * (int64_t)n) return kTabInput;
    *log = alog, *used = (uint32_t)((pos + 7) >> 3);
    return kTabOk;
}

// norm[0, max_symbol] (max_symbol < kFseSymbols) to table[0, 1 << log), log <= 9; next: max_symbol + 1 words of
// work. The counts are checked again here: with a sum that is not 1 << log nothing is written.
OXH_ZSTD_BOTH uint32_t fse_build(const int16_t* norm, uint32_t max_symbol, uint32_t log, FseCell* table, uint16_t* next) {
    const uint32_t size = 1u << log;
    uint32_t sum = 0;
    for (uint32_t s = 0; s <= max_symbol; ++s) sum += norm[s] < 0 ? 1u : (uint32_t)norm[s];
    if (log > 9 || sum != size) return sum > size ? kTabOverrun : kTabUnderrun;
    uint32_t high = size;
    for (uint32_t s = 0; s <= max_symbol; ++s) {
        next[s] = norm[s] < 0 ? 1 : (uint16_t)norm[s];
        if (norm[s] < 0) table[--high].symbol = (uint8_t)s;  // "less than 1": a cell at the end
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t pos = 0;
    for (uint32_t s = 0; s <= max_symbol; ++s)
        for (int32_t k = 0; k < norm[s]; ++k) {
            table[pos].symbol = (uint8_t)s;
            do pos = (pos + step) & mask;  // (step is odd: every cell is met)
            while (pos >= high);
        }
    for (uint32_t c = 0; c < size; ++c) {
        const uint32_t x = next[table[c].symbol]++;  // size > x > 0
        const uint32_t nbits = log - high_bit(x);
        table[c].nbits = (uint8_t)nbits, table[c].base = (uint16_t)((x << nbits) - size);
    }
    return kTabOk;
}

// The predefined distributions (RFC 8878, 3.1.1.3.2.2) and the codes' baselines and extra bits (3.1.1.3.2.1.1).
OXH_ZSTD_BOTH void predefined_counts(uint32_t kind, int16_t* norm, uint32_t* log) {  // kind 0 LL, 1 OF, 2 ML
    const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    if (kind == 0) {
        for (uint32_t s = 0; s <= kMaxLL; ++s) norm[s] = ll[s];
        *log = 6;
    } else if (kind == 1) {
        for (uint32_t s = 0; s <= kMaxOF; ++s) norm[s] = s < 29 ? of[s] : 0;
        *log = 5;
    } else {
        for (uint32_t s = 0; s <= kMaxML; ++s) norm[s] = ml[s];
        *log = 6;
    }
}
OXH_ZSTD_BOTH uint32_t ll_bits(uint32_t code) { return code < 16 ? 0 : code < 20 ? 1 : code < 22 ? 2 : code < 24 ? 3 : code == 24 ? 4 : code - 19; }
OXH_ZSTD_BOTH uint32_t ll_base(uint32_t code) {
    return code < 16 ? code : code < 20 ? 16 + 2 * (code - 16) : code == 20 ? 24 : code == 21 ? 28 : code == 22 ? 32 : code == 23 ? 40 : code == 24 ? 48
                                                                                                                                     : 1u << (code - 19);
}
OXH_ZSTD_BOTH uint32_t ml_bits(uint32_t code) {
    return code < 32 ? 0 : code < 36 ? 1 : code < 38 ? 2 : code < 40 ? 3 : code < 42 ? 4 : code < 43 ? 5 : code - 36;
}
OXH_ZSTD_BOTH uint32_t ml_base(uint32_t code) {
    return code < 32 ? code + 3 : code < 36 ? 35 + 2 * (code - 32) : code == 36 ? 43 : code == 37 ? 47 : code == 38 ? 51 : code == 39 ? 59
           : code == 40 ? 67 : code == 41 ? 83 : code == 42 ? 99 : 3 + (1u << (code - 36));
}

// A Huffman tree description at src[0, n) to weights[0, *count) (weights: 256 bytes; the last, implied weight is
// huf_build's to add) and *used, its bytes. work: kFseSymbols int16 + kFseSymbols uint16 + 64 FseCell, in this order.
OXH_ZSTD_BOTH uint32_t huf_read_weights(const uint8_t* src, uint32_t n, uint8_t* weights, uint32_t* count, uint32_t* used, void* work) {
    if (n == 0) return kTabInput;
    const uint32_t head = src[0];
    if (head >= 128) {  // direct: 4 bits each
        const uint32_t nw = head - 127, bytes = (nw + 1) / 2;
        if (bytes > n - 1) return kTabInput;
        for (uint32_t k = 0; k < nw; ++k) weights[k] = (k & 1) ? src[1 + k / 2] & 15 : src[1 + k / 2] >> 4;
        *count = nw, *used = 1 + bytes;
        return kTabOk;
    }
    if (head == 0 || head > n - 1) return kTabInput;
    int16_t* norm = (int16_t*)work;
    uint16_t* next = (uint16_t*)(norm + kFseSymbols);
    FseCell* table = (FseCell*)(next + kFseSymbols);
    uint32_t log = 0, at = 0;
    uint32_t rc = fse_read_counts(src + 1, head, kLogWeights, kMaxWeight, norm, &log, &at);
    if (rc == kTabOk) rc = fse_build(norm, kMaxWeight, log, table, next);
    if (rc) return rc;
    BackBits b;
    if (!back_open(b, src + 1 + at, head - at)) return kTabWeights;
    uint32_t s1 = back_read(b, log), s2 = back_read(b, log), nw = 0;
    if (b.left < 0) return kTabWeights;
    while (true) {  // two states in turn, until one asks for more than there is: the other's symbol is the last
        if (nw + 2 > 255) return kTabWeights;
        weights[nw++] = table[s1].symbol;
        s1 = table[s1].base + back_read(b, table[s1].nbits);
        if (b.left < 0) {
            weights[nw++] = table[s2].symbol;
            break;
        }
        const uint32_t t = s1;
        s1 = s2, s2 = t;
    }
    *count = nw, *used = 1 + head;
    return kTabOk;
}

// weights[0, count), count <= 255, to table[0, 1 << *log): a cell is symbol | nbits << 8, indexed by the stream's next
// *log bits; weights[count] becomes the implied last weight. rank: 16 words of work.
OXH_ZSTD_BOTH uint32_t huf_build(uint8_t* weights, uint32_t count, uint16_t* table, uint32_t* log, uint32_t* rank) {
    if (count == 0 || count > 255) return kTabWeights;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < count; ++k) {
        if (weights[k] > kMaxWeight) return kTabWeights;
        sum += weights[k] ? 1u << (weights[k] - 1) : 0;
    }
    if (sum == 0) return kTabSum;
    const uint32_t bits = high_bit(sum) + 1, left = (1u << bits) - sum;  // sum < 2^bits <= 2 sum
    if (bits > kMaxWeight || (left & (left - 1))) return kTabSum;
    weights[count] = (uint8_t)(high_bit(left) + 1);
    for (uint32_t w = 0; w < 16; ++w) rank[w] = 0;
    for (uint32_t k = 0; k <= count; ++k) rank[weights[k]] += 1;
    uint32_t at = 0;  // weight 1 (the longest codes) first; a symbol of weight w fills 2^(w - 1) cells
    for (uint32_t w = 1; w <= bits; ++w) {
        const uint32_t cells = rank[w] << (w - 1);
        rank[w] = at, at += cells;
    }
    for (uint32_t k = 0; k <= count; ++k) {
        const uint32_t w = weights[k];
        if (!w) continue;
        const uint32_t cells = 1u << (w - 1), cell = k | (bits + 1 - w) << 8;
        for (uint32_t c = 0; c < cells; ++c) table[rank[w] + c] = (uint16_t)cell;  // the sum is 2^bits: inside the table
        rank[w] += cells;
    }
    *log = bits;
    return kTabOk;
}

// One Huffman stream src[0, n) to out[0, count). false: no stream, or one that is not consumed to its first bit.
OXH_ZSTD_BOTH bool huf_decode_stream(const uint8_t* src, uint32_t n, const uint16_t* table, uint32_t log, uint8_t* out, uint32_t count) {
    BackBits b;
    if (!back_open(b, src, n)) return false;
    uint32_t done = 0;
    while (done < count) {  // 56 bits a refill, the next code at the top: five codes of at most 11 bits
        uint64_t c = ((uint64_t)bits_at(src, n, b.left - 28, 28) << 28 | bits_at(src, n, b.left - 56, 28)) << 8;
        for (uint32_t k = 0; k < 5 && done < count; ++k) {
            const uint32_t cell = table[c >> (64 - log)], nbits = cell >> 8;  // 1 <= nbits <= log
            c <<= nbits, b.left -= nbits;
            out[done++] = (uint8_t)cell;
        }
    }
    return b.left == 0;
}

// A literals section's header at src[0, n): type 0 Raw, 1 RLE, 2 Huffman, 3 treeless; streams 1 or 4; regen, the
// literals' bytes; comp, the section's bytes behind the header (types 2 and 3); bytes, the header's.
struct LitHeader {
    uint32_t type, streams, regen, comp, bytes;
};
OXH_ZSTD_BOTH bool lit_header(const uint8_t* src, uint32_t n, LitHeader& h) {
    if (n == 0) return false;
    const uint32_t form = (src[0] >> 2) & 3;
    h.type = src[0] & 3, h.streams = 1, h.comp = 0;
    h.bytes = h.type < 2 ? (form == 1 ? 2 : form == 3 ? 3 : 1) : (form < 2 ? 3 : form + 2);
    if (h.bytes > n) return false;
    uint64_t v = 0;
    for (uint32_t k = 0; k < h.bytes; ++k) v |= (uint64_t)src[k] << (8 * k);
    if (h.type < 2) {
        h.regen = (uint32_t)(v >> (form == 1 || form == 3 ? 4 : 3));
    } else {
        const uint32_t width = form < 2 ? 10 : form == 2 ? 14 : 18;
        h.regen = (uint32_t)(v >> 4) & ((1u << width) - 1), h.comp = (uint32_t)(v >> (4 + width)) & ((1u << width) - 1);
        h.streams = form == 0 ? 1 : 4;
    }
    return true;
}

// A sequences section's count at src[0, n) and the count's bytes.
OXH_ZSTD_BOTH bool seq_count(const uint8_t* src, uint32_t n, uint32_t* count, uint32_t* bytes) {
    if (n == 0) return false;
    const uint32_t b0 = src[0];
    *bytes = b0 < 128 ? 1 : b0 < 255 ? 2 : 3;
    if (*bytes > n) return false;
    *count = b0 < 128 ? b0 : b0 < 255 ? ((b0 - 128) << 8) + src[1] : src[1] + ((uint32_t)src[2] << 8) + 0x7F00;
    return true;
}

// The three interleaved FSE states over the sequences' bitstream. A table of log 0 is one cell (the RLE mode).
struct SeqTables {
    const FseCell *ll, *of, *ml;
    uint32_t ll_log, of_log, ml_log;
};
struct SeqState {
    BackBits b;
    uint32_t ll, of, ml;
};
OXH_ZSTD_BOTH bool seq_open(SeqState& s, const uint8_t* src, uint32_t n, const SeqTables& t) {
    if (!back_open(s.b, src, n)) return false;
    s.ll = back_read(s.b, t.ll_log), s.of = back_read(s.b, t.of_log), s.ml = back_read(s.b, t.ml_log);
    return s.b.left >= 0;
}
// The next sequence: its literal length, match length and offset value (the repeat offsets not resolved). The
// caller looks at s.b.left: below 0, the stream has ended before the sequence did.
OXH_ZSTD_BOTH void seq_next(SeqState& s, const SeqTables& t, bool last, uint32_t* ll, uint32_t* ml, uint64_t* offset_value) {
    const FseCell cl = t.ll[s.ll], co = t.of[s.of], cm = t.ml[s.ml];  // symbols inside their alphabets: the builders'
    *offset_value = (1ull << co.symbol) + back_read(s.b, co.symbol);
    *ml = ml_base(cm.symbol) + back_read(s.b, ml_bits(cm.symbol));
    *ll = ll_base(cl.symbol) + back_read(s.b, ll_bits(cl.symbol));
    if (last) return;
    s.ll = cl.base + back_read(s.b, cl.nbits);
    s.ml = cm.base + back_read(s.b, cm.nbits);
    s.of = co.base + back_read(s.b, co.nbits);
}

// The offset an offset value names, with the three repeat offsets brought up to date; 0: an offset of 0 (refused).
struct Repeats {
    uint64_t r0, r1, r2;
};
OXH_ZSTD_BOTH uint64_t resolve_offset(Repeats& r, uint64_t offset_value, uint32_t ll) {
    if (offset_value > 3) {
        r.r2 = r.r1, r.r1 = r.r0, r.r0 = offset_value - 3;
        return r.r0;
    }
    const uint32_t which = (uint32_t)offset_value - 1 + (ll == 0);  // a literal length of 0 shifts the meaning by one
    if (which == 0) return r.r0;
    const uint64_t off = which == 1 ? r.r1 : which == 2 ? r.r2 : r.r0 - 1;
    if (off == 0) return 0;
    if (which != 1) r.r2 = r.r1;
    r.r1 = r.r0, r.r0 = off;
    return off;
}

}  // namespace oxh::zst
