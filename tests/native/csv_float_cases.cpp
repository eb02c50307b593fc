// tests/native/csv_float_cases.cpp -- the CSV float conversions of csv_number.hpp and csv_text.hpp (the code the
// kernels of csv_read.hip and csv_write.hip compile) over cells that a test sends in, one answer per cell on stdout:
//   csv_float_cases read  < one text per line     "N" (not the grammar), "X <bits>" (parse_float's exact kinds and the
//                                                 words: exact_value's bits) or "D <bits>" (deferred: the host's
//                                                 conversion of the text, csv_host.hpp)
//   csv_float_cases write < 8-byte doubles        "X <text>" (float_form / form_text) or "D <text>" (deferred: the
//                                                 host's slot)
// tests/test_csv_floats_cpu.py compares every line with the restatements of tests/_csv.py and tests/_csvwrite.py.
// Built by oxen_amd/build.py (build_host); the test also builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../oxen_amd/csrc/csv_host.hpp"
#include "../../oxen_amd/csrc/csv_text.hpp"

namespace num = oxh::csvnum;
namespace text = oxh::csvtext;

static const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

static uint64_t bits_of(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

static int read_cases() {
    std::string line;
    for (int c = 0; c != EOF;) {
        line.clear();
        while ((c = std::getchar()) != EOF && c != '\n') line.push_back((char)c);
        if (c == EOF && line.empty()) break;
        const std::vector<uint8_t> cell(line.begin(), line.end());  // a heap block of exactly the cell: a read past it is the sanitizer's
        uint64_t m;
        int32_t e10;
        bool neg;
        const uint32_t kind = num::parse_float(cell.data(), (uint32_t)cell.size(), m, e10, neg);
        if (kind == num::kFloatNoMatch)
            std::puts("N");
        else if (kind == num::kFloatDeferred)
            std::printf("D %016llx\n", (unsigned long long)bits_of(oxh::csv::convert_deferred(line.data(), line.size())));
        else if (kind == num::kFloatExact)
            std::printf("X %016llx\n", (unsigned long long)bits_of(num::exact_value(m, e10, neg, kPow10)));
        else
            std::printf("X %016llx\n", (unsigned long long)((kind == num::kFloatInf ? num::kInfBits : num::kQuietNan) | (neg ? num::kSignBit : 0)));
    }
    return 0;
}

static int write_cases() {
    uint64_t bits;
    while (std::fread(&bits, 8, 1, stdin) == 1) {
        uint8_t buf[text::kDeferSlot + 8];
        std::memset(buf, '#', sizeof buf);
        const text::FloatForm f = text::float_form(bits, kPow10);
        uint32_t n;
        if (f.kind == text::kFormDeferred) {
            text::deferred_slot(bits, buf);
            n = buf[text::kDeferSlot - 1];
        } else {
            n = text::form_text(f, nullptr);
            if (text::form_text(f, buf) != n || buf[n] != '#') {
                std::fprintf(stderr, "%016llx: the measured and the written text differ\n", (unsigned long long)bits);
                return 1;
            }
        }
        std::printf("%c %.*s\n", f.kind == text::kFormDeferred ? 'D' : 'X', (int)n, (const char*)buf);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "read")) return read_cases();
    if (argc == 2 && !std::strcmp(argv[1], "write")) return write_cases();
    std::fprintf(stderr, "usage: csv_float_cases read|write < cells\n");
    return 2;
}
