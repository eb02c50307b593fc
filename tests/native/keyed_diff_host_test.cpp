// tests/native/keyed_diff_host_test.cpp -- the host-only pieces of oxh_keyed_diff_* (oxen_amd/csrc/
// keyed_diff_host.hpp) in a program of their own: the argument checks in the header's order and the
// ordering of a left row's pairs. No HIP and no library: g++ -std=c++17 (add -fsanitize=address,undefined
// for a sanitizer run). Prints "ok" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstring>
#include <random>

#include "../../oxen_amd/csrc/keyed_diff_host.hpp"

using namespace oxh::keyed;

static int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static bool says(const char* got, const char* part) { return got && std::strstr(got, part); }

static void arguments() {
    std::vector<uint64_t> keys(2 * 8), targets(2 * 8);
    uint64_t bits[2] = {0, 0}, counts[8] = {};
    uint32_t left[4] = {}, right[4] = {};
    uint8_t status[4] = {};
    const uint64_t *k = keys.data(), *t = targets.data();
    EXPECT(!argument_error(k, 8, k, 8, t, t, bits, 0, 4, left, right, status, counts));
    EXPECT(!argument_error(k, 8, k, 8, nullptr, nullptr, bits, 1, 0, nullptr, nullptr, nullptr, counts));
    EXPECT(!argument_error(nullptr, 0, nullptr, 0, nullptr, nullptr, bits, 0, 0, nullptr, nullptr, nullptr, counts));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 0, 4, left, right, status, nullptr), "counts8"));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, nullptr, 0, 4, left, right, status, counts), "bit_offsets2"));
    EXPECT(says(argument_error(k, 0xFFFFFFFFull, k, 8, t, t, bits, 0, 4, left, right, status, counts), "2^32 - 2"));
    EXPECT(says(argument_error(k, 8, k, 0xFFFFFFFFull, t, t, bits, 0, 4, left, right, status, counts), "2^32 - 2"));
    EXPECT(says(argument_error(nullptr, 8, k, 8, t, t, bits, 0, 4, left, right, status, counts), "key table"));
    EXPECT(says(argument_error(k, 8, nullptr, 8, t, t, bits, 0, 4, left, right, status, counts), "key table"));
    // the same table as keys and targets is fine; one that starts inside the other is not
    EXPECT(!argument_error(k, 8, k, 8, k, k, bits, 0, 4, left, right, status, counts));
    EXPECT(says(argument_error(k, 4, k, 8, k + 2, t, bits, 0, 4, left, right, status, counts), "overlaps"));
    EXPECT(says(argument_error(k + 6, 4, k, 8, k, t, bits, 0, 4, left, right, status, counts), "overlaps"));
    EXPECT(says(argument_error(k, 8, k, 4, t, k + 7, bits, 0, 4, left, right, status, counts), "overlaps"));
    EXPECT(!argument_error(k, 4, k, 8, k + 8, t, bits, 0, 4, left, right, status, counts));   // behind its last row
    EXPECT(!argument_error(k, 0, k, 8, k + 2, t, bits, 0, 4, left, right, status, counts));   // a side without rows
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 0, 4, nullptr, right, status, counts), "capacity"));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 0, 4, left, nullptr, status, counts), "capacity"));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 0, 4, left, right, nullptr, counts), "capacity"));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 2, 4, left, right, status, counts), "flag"));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 0x80000001u, 4, left, right, status, counts), "flag"));
    // the order: a NULL counts8 before everything, rows before tables, tables before outputs, outputs before flags
    EXPECT(says(argument_error(nullptr, 0xFFFFFFFFull, k, 8, t, t, bits, 2, 4, nullptr, right, status, nullptr), "counts8"));
    EXPECT(says(argument_error(nullptr, 0xFFFFFFFFull, k, 8, t, t, bits, 2, 4, nullptr, right, status, counts), "2^32 - 2"));
    EXPECT(says(argument_error(nullptr, 8, k, 8, t, t, bits, 2, 4, nullptr, right, status, counts), "key table"));
    EXPECT(says(argument_error(k, 8, k, 8, t, t, bits, 2, 4, nullptr, right, status, counts), "capacity"));
}

static void sorting() {
    // runs: left 0 (one pair), left 1 (three, shuffled), left 2 (l, none), left 3 (two), then right-only rows
    uint32_t left[] = {0, 1, 1, 1, 2, 3, 3, kNone, kNone, kNone};
    uint32_t right[] = {5, 9, 2, 7, kNone, 8, 1, 3, 4, 6};
    uint8_t status[] = {0, 3, 1, 2, 2, 3, 0, 1, 1, 1};
    sort_runs(left, right, status, 10);
    const uint32_t want_right[] = {5, 2, 7, 9, kNone, 1, 8, 3, 4, 6};
    const uint8_t want_status[] = {0, 1, 2, 3, 2, 0, 3, 1, 1, 1};
    EXPECT(!std::memcmp(right, want_right, sizeof right) && !std::memcmp(status, want_status, sizeof status));
    sort_runs(left, right, status, 0);       // nothing to do
    sort_runs(left, right, status, 1);
    EXPECT(right[0] == 5);
    // one long shuffled run between two short ones: the statuses follow their rows
    const uint32_t n = 3000;
    std::vector<uint32_t> l(n + 2, 7), r(n + 2);
    std::vector<uint8_t> s(n + 2);
    for (uint32_t i = 0; i < n + 2; ++i) r[i] = i;
    std::mt19937 rng(5);
    std::shuffle(r.begin() + 1, r.end() - 1, rng);
    l[0] = 6, r[0] = 4000, l[n + 1] = 8, r[n + 1] = 0;
    for (uint32_t i = 0; i < n + 2; ++i) s[i] = (uint8_t)(r[i] % 4);
    sort_runs(l.data(), r.data(), s.data(), n + 2);
    EXPECT(r[0] == 4000 && r[n + 1] == 0);
    for (uint32_t i = 1; i <= n; ++i) EXPECT(r[i] == i && s[i] == i % 4);
}

int main() {
    arguments();
    sorting();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
