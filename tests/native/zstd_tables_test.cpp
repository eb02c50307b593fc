// tests/native/zstd_tables_test.cpp -- oxen_amd/csrc/zstd_tables.hpp on the CPU, plain and under ASan / UBSan
// (tests/test_parquet_zstd_cpu.py): the predefined distributions against the first and last rows of RFC 8878's
// appendix A; one real FSE description and one real Huffman tree description (bytes of tests/golden/zstd/
// words_900_l3.zst at 330 and 13); hostile descriptions, each of which must return its cause; and the bound of
// parquet_read_host.hpp on what a ZSTD page may claim, at its edge. Every table and work
// array is a heap block of exactly the size the header states, so that a write outside it stops the sanitised run.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../oxen_amd/csrc/parquet_read_host.hpp"
#include "../../oxen_amd/csrc/zstd_tables.hpp"

using namespace oxh::zst;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("line %d: %s\n", __LINE__, #cond);           \
            ++failures;                                              \
        }                                                            \
    } while (0)

struct Fse {
    std::unique_ptr<int16_t[]> norm;
    std::unique_ptr<uint16_t[]> next;
    std::unique_ptr<FseCell[]> table;
    uint32_t log = 0, used = 0;
    Fse(uint32_t max_symbol, uint32_t max_log) : norm(new int16_t[max_symbol + 1]), next(new uint16_t[max_symbol + 1]), table(new FseCell[1u << max_log]) {}
};

static bool row(const FseCell& c, uint32_t symbol, uint32_t nbits, uint32_t base) { return c.symbol == symbol && c.nbits == nbits && c.base == base; }

static uint32_t read_and_build(const std::vector<uint8_t>& bytes, uint32_t max_symbol, uint32_t max_log, Fse& f) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[bytes.size()]);  // exactly the description: a read behind it is seen
    for (size_t k = 0; k < bytes.size(); ++k) src[k] = bytes[k];
    uint32_t rc = fse_read_counts(src.get(), (uint32_t)bytes.size(), max_log, max_symbol, f.norm.get(), &f.log, &f.used);
    return rc ? rc : fse_build(f.norm.get(), max_symbol, f.log, f.table.get(), f.next.get());
}

static uint32_t weights_to_table(std::vector<uint8_t> given, uint32_t* log) {
    std::unique_ptr<uint8_t[]> weights(new uint8_t[256]);
    std::unique_ptr<uint16_t[]> table(new uint16_t[kHufCells]);
    std::unique_ptr<uint32_t[]> rank(new uint32_t[16]);
    for (size_t k = 0; k < given.size() && k < 256; ++k) weights[k] = given[k];
    return huf_build(weights.get(), (uint32_t)given.size(), table.get(), log, rank.get());
}

int main() {
    {  // the predefined distributions: appendix A's first and last rows
        Fse ll(kMaxLL, kLogLL), of(kMaxOF, kLogOF), ml(kMaxML, kLogML);
        predefined_counts(0, ll.norm.get(), &ll.log);
        predefined_counts(1, of.norm.get(), &of.log);
        predefined_counts(2, ml.norm.get(), &ml.log);
        CHECK(ll.log == 6 && of.log == 5 && ml.log == 6);
        CHECK(fse_build(ll.norm.get(), kMaxLL, 6, ll.table.get(), ll.next.get()) == kTabOk);
        CHECK(fse_build(of.norm.get(), kMaxOF, 5, of.table.get(), of.next.get()) == kTabOk);
        CHECK(fse_build(ml.norm.get(), kMaxML, 6, ml.table.get(), ml.next.get()) == kTabOk);
        CHECK(row(ll.table[0], 0, 4, 0) && row(ll.table[1], 0, 4, 16) && row(ll.table[2], 1, 5, 32) && row(ll.table[63], 32, 6, 0));
        CHECK(row(of.table[0], 0, 5, 0) && row(of.table[1], 6, 4, 0) && row(of.table[31], 24, 5, 0));
        CHECK(row(ml.table[0], 0, 6, 0) && row(ml.table[1], 1, 4, 0) && row(ml.table[63], 46, 6, 0));
        CHECK(ll_base(15) == 15 && ll_bits(15) == 0 && ll_base(16) == 16 && ll_bits(19) == 1 && ll_base(24) == 48 && ll_bits(24) == 4 && ll_base(25) == 64 &&
              ll_bits(25) == 6 && ll_base(35) == 65536 && ll_bits(35) == 16);
        CHECK(ml_base(0) == 3 && ml_base(31) == 34 && ml_base(32) == 35 && ml_bits(35) == 1 && ml_base(42) == 99 && ml_bits(42) == 5 && ml_base(43) == 131 &&
              ml_bits(43) == 7 && ml_base(52) == 65539 && ml_bits(52) == 16);
    }
    {  // a real offset-code description: every cell's symbol is in the alphabet and a symbol has as many cells as its count
        Fse f(kMaxOF, kLogOF);
        CHECK(read_and_build({0x10, 0x14, 0x82, 0x18, 0xc4, 0x07, 0xc1, 0xd0, 0xdb, 0xdc, 0xe0, 0x2b, 0x98, 0xfb, 0x89}, kMaxOF, kLogOF, f) == kTabOk);
        CHECK(f.log >= 5 && f.log <= kLogOF && f.used > 1 && f.used < 15);
        uint32_t cells[kMaxOF + 1] = {};
        for (uint32_t c = 0; c < (1u << f.log); ++c) {
            CHECK(f.table[c].symbol <= kMaxOF && f.table[c].nbits <= f.log && f.table[c].base + (1u << f.table[c].nbits) <= (1u << f.log));
            if (f.table[c].symbol <= kMaxOF) cells[f.table[c].symbol] += 1;
        }
        for (uint32_t s = 0; s <= kMaxOF; ++s) CHECK(cells[s] == (f.norm[s] < 0 ? 1u : (uint32_t)f.norm[s]));
    }
    {  // a real tree description (FSE-compressed weights): the code lengths fill the table exactly (Kraft's equality)
        const uint8_t tree[21] = {0x14, 0xa0, 0x55, 0x07, 0x24, 0x49, 0x92, 0x24, 0xa1, 0x24, 0xfa, 0x56, 0xb2, 0xfe, 0x76, 0x00, 0x00, 0x88, 0xa8, 0xfa, 0x1a};
        std::unique_ptr<uint8_t[]> src(new uint8_t[21]), weights(new uint8_t[256]), work(new uint8_t[2 * 2 * kFseSymbols + 64 * sizeof(FseCell)]);
        std::unique_ptr<uint16_t[]> table(new uint16_t[kHufCells]);
        std::unique_ptr<uint32_t[]> rank(new uint32_t[16]);
        for (int k = 0; k < 21; ++k) src[k] = tree[k];
        uint32_t count = 0, used = 0, log = 0;
        CHECK(huf_read_weights(src.get(), 21, weights.get(), &count, &used, work.get()) == kTabOk && used == 21 && count >= 97 && count <= 255);
        CHECK(huf_build(weights.get(), count, table.get(), &log, rank.get()) == kTabOk && log >= 1 && log <= kMaxWeight);
        uint32_t filled[256] = {};
        for (uint32_t c = 0; c < (1u << log); ++c) {
            const uint32_t symbol = table[c] & 255, nbits = table[c] >> 8;
            CHECK(symbol <= count && nbits >= 1 && nbits <= log && weights[symbol] == log + 1 - nbits);
            filled[symbol] += 1;
        }
        for (uint32_t s = 0; s <= count; ++s) CHECK(filled[s] == (weights[s] ? 1u << (weights[s] - 1) : 0u));
        CHECK(weights[' '] >= weights['q']);  // the text's most frequent byte has no longer a code than a rare letter
        const uint8_t direct[4] = {0x82, 0x12, 0x10, 0x00};  // direct: 3 weights of 4 bits, 1 2 1
        CHECK(huf_read_weights(direct, 3, weights.get(), &count, &used, work.get()) == kTabOk && count == 3 && used == 3 && weights[0] == 1 && weights[1] == 2 && weights[2] == 1);
        CHECK(huf_read_weights(direct, 2, weights.get(), &count, &used, work.get()) == kTabInput);
    }
    {  // hostile descriptions
        Fse f(kMaxOF, kLogOF);
        CHECK(read_and_build({0x04, 0xFF, 0xFF}, kMaxOF, kLogOF, f) == kTabLog);  // accuracy log 9 for offsets
        Fse wide(kMaxLL, kLogLL);
        CHECK(read_and_build({0x0F}, kMaxLL, kLogLL, wide) == kTabLog);           // accuracy log 20
        // counts that overrun and that underrun the total, and a log above the builder's: nothing is written
        for (uint32_t s = 0; s <= kMaxOF; ++s) f.norm[s] = 2;
        CHECK(fse_build(f.norm.get(), kMaxOF, 5, f.table.get(), f.next.get()) == kTabOverrun);
        for (uint32_t s = 0; s <= kMaxOF; ++s) f.norm[s] = s < 3 ? -1 : 0;
        CHECK(fse_build(f.norm.get(), kMaxOF, 5, f.table.get(), f.next.get()) == kTabUnderrun);
        CHECK(fse_build(f.norm.get(), kMaxOF, 10, f.table.get(), f.next.get()) != kTabOk);
        // log 5 and "less than 1" for every symbol (value 0 in 5 bits each): 32 symbols spend 32, the alphabet of 4 ends first
        Fse small(3, 5);
        CHECK(read_and_build({0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, 3, 5, small) == kTabUnderrun);
        // log 5, probability 0 (value 1) and the repeat flag 3 again and again: zeros past the alphabet
        CHECK(read_and_build({0x10, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF}, kMaxOF, kLogOF, f) == kTabRepeat);
        CHECK(read_and_build({0x10}, kMaxOF, kLogOF, f) == kTabInput);  // the description ends in its first symbol
        uint32_t log = 0;
        CHECK(weights_to_table({1, 1, 1}, &log) == kTabOk && log == 2);      // 3 and the implied weight 1: 4
        CHECK(weights_to_table({2, 1, 2, 1}, &log) == kTabOk && log == 3);   // 6 and the implied weight 2: 8
        CHECK(weights_to_table({2, 2, 1}, &log) == kTabSum);                 // 5 of 8: the 3 that are left are no power of two
        CHECK(weights_to_table({12, 1}, &log) == kTabWeights);               // a weight above 11
        CHECK(weights_to_table({0, 0, 0}, &log) == kTabSum);                 // no weight at all
        CHECK(weights_to_table({11, 11}, &log) == kTabSum);                  // 2^11 already: the last symbol would make codes of 12 bits
        CHECK(weights_to_table(std::vector<uint8_t>(256, 1), &log) == kTabWeights);  // 256 symbols and the implied one
        CHECK(weights_to_table(std::vector<uint8_t>(255, 1), &log) == kTabOk && log == 8);  // 255 and the implied one: the largest alphabet
    }
    {  // a ZSTD page: 5 bytes of frame header, then 128 KiB for every 3 bytes; the image's plan applies it to ZSTD pages only
        namespace pr = oxh::pqr;
        CHECK(!pr::zstd_size_plausible(4, 0) && pr::zstd_size_plausible(5, 0) && !pr::zstd_size_plausible(7, 1) && pr::zstd_size_plausible(8, 131072) &&
              !pr::zstd_size_plausible(8, 131073) && pr::zstd_size_plausible(11, 262144) && !pr::zstd_size_plausible(11, 262145));
        std::vector<pr::PageRec> recs(2);
        recs[0] = pr::PageRec{100, 131072, 0, 1, 0, 0, 0, 0, pr::kPageInImage | pr::kPageZstd, 9, 0};  // an RLE block: Snappy's bound would refuse it
        recs[1] = pr::PageRec{200, 131072, 0, 1, 0, 0, 0, 0, pr::kPageInImage, 9, 0};
        CHECK(pr::plan_image(recs).implausible == 1);
        recs[1].flags |= pr::kPageZstd, recs[1].body_size = 131073;
        CHECK(pr::plan_image(recs).implausible == 1);
        recs[1].body_size = 100;
        CHECK(pr::plan_image(recs).implausible == ~0ull && pr::plan_image(recs).pages == 2);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
