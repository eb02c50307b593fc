// tests/native/cdc_plan_test.cpp -- the FastCDC section planner (oxen_amd/csrc/fastcdc_plan.hpp) on the
// CPU: the path (scan or walk), section size, warm-up, list capacities and the section table of
// planned calls, the four error texts, and the planner's invariants over a small lattice. The 4 GiB
// window rule guards W's 32-bit buffer offsets and cannot be reached from a GPU test without an arena
// above 4 GiB; here it is two integers. Built by oxen_amd/build.py (build_host), run by
// tests/test_cdc_plan.py. Exit status 0 = every check passed.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../oxen_amd/csrc/fastcdc_plan.hpp"

namespace {

int g_failed = 0, g_checks = 0;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        ++g_checks;                                           \
        if (!(cond)) {                                        \
            ++g_failed;                                       \
            fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
        }                                                     \
    } while (0)

constexpr uint64_t KiB = 1024, MiB = 1024 * KiB, GiB = 1024 * MiB;
constexpr int kCus = 256, kLds = 160 * 1024;

struct Call {
    std::vector<uint64_t> off, len;
    uint32_t mn = 4096, av = 8192, mx = 16384, lv = 1;
    uint64_t addr = 0x7f0000000000ull;  // 128-B aligned
    int walk_env = -1;
    long long sec_env = -1, warmup_env = -1;
    int cap_env = -1;
    int cus = kCus, lds = kLds;
};

Call one_file(uint64_t len) {
    Call c;
    c.off = {0};
    c.len = {len};
    return c;
}

int run(const Call& c, oxh::CdcPlan& p) {
    const oxh::CdcPlanInput in{c.off.data(), c.len.data(), c.len.size(), c.mn, c.av, c.mx, c.lv, c.addr, c.cus, c.lds,
                               c.walk_env, c.sec_env, c.warmup_env, c.cap_env};
    return oxh::cdc_plan(in, p);
}

// the path and the section geometry of a call that must plan
void expect(const char* name, const Call& c, bool walk, uint64_t sec, long long warmup, long long cap, long long speccap,
            long long n_sec, const std::vector<uint64_t>& sec_base = {}) {
    oxh::CdcPlan p;
    const int rc = run(c, p);
    CHECK(rc == OXH_OK, "%s: rc %d (%s)", name, rc, p.error.c_str());
    if (rc != OXH_OK) return;
    CHECK(p.walk == walk, "%s: path %s", name, p.walk ? "walk" : "scan");
    CHECK(p.prm.sec == sec, "%s: sec %" PRIu64, name, p.prm.sec);
    CHECK(p.prm.unit == p.prm.sec / 64, "%s: unit %" PRIu64, name, p.prm.unit);
    if (warmup >= 0) CHECK(p.prm.warmup == (uint64_t)warmup, "%s: warm-up %" PRIu64, name, p.prm.warmup);
    if (cap >= 0) CHECK(p.prm.cap == (uint32_t)cap, "%s: cap %u", name, p.prm.cap);
    if (speccap >= 0) CHECK(p.prm.speccap == (uint32_t)speccap, "%s: speccap %u", name, p.prm.speccap);
    if (n_sec >= 0) CHECK(p.n_sec == (uint64_t)n_sec, "%s: n_sec %" PRIu64, name, p.n_sec);
    if (!sec_base.empty()) {
        CHECK(p.sec_base == sec_base, "%s: sec_base[0..%zu) differs, last %" PRIu64, name, p.sec_base.size(),
              p.sec_base.empty() ? 0 : p.sec_base.back());
    }
    CHECK(p.prm.min == c.mn && p.prm.avg == c.av && p.prm.max == c.mx, "%s: sizes not carried over", name);
}

void expect_error(const char* name, const Call& c, const char* text) {
    oxh::CdcPlan p;
    const int rc = run(c, p);
    CHECK(rc == OXH_ERR_INVALID, "%s: rc %d", name, rc);
    const size_t n = strlen(text);
    CHECK(p.error.size() >= n && p.error.compare(p.error.size() - n, n, text) == 0, "%s: error text '%s'", name,
          p.error.c_str());
}

void table() {
    {  // A: avg above 16 KiB takes the scan, 8 max-sized chunks per section
        Call c = one_file(3 * MiB);
        c.mn = 4096, c.av = 65536, c.mx = 131072;
        expect("A", c, false, 1048576, 786432, 16, 290, 3);
    }
    const Call B = one_file(1 * MiB);
    expect("B", B, true, 65536, 32768, 10, 22, 16);
    {  // C: an arena 64 bytes off a 128-B line cannot take the walk
        Call c = B;
        c.addr += 64;
        expect("C", c, false, 524288, 131072, 24, 134, 2);
    }
    {  // D: one wave's 64 sections would span more than 4 GiB - 1 MiB: the scan, with its own plan
        Call c = B;
        c.off = {0, 5 * GiB};
        c.len = {1 * MiB, 1 * MiB};
        expect("D", c, false, 524288, 131072, 24, 134, 4, {0, 2, 4});
        c.walk_env = 1;
        expect_error("D'", c, "a wave's sections span 4 GiB");
        oxh::CdcPlan p;
        run(c, p);
        CHECK(p.error == "OXH_CDC_WALK=1: a wave's sections span 4 GiB", "D': '%s'", p.error.c_str());
    }
    {  // E: a 128 MiB section's start lists do not fit X's LDS
        Call c = B;
        c.sec_env = 128 * (long long)MiB;
        expect("E", c, false, 134217728, -1, 4104, 32774, 1);
        c.walk_env = 1;
        expect_error("E'", c, "X's section lists do not fit the workgroup's LDS");
        oxh::CdcPlan p;
        run(c, p);
        CHECK(p.error == "OXH_CDC_WALK=1: X's section lists do not fit the workgroup's LDS", "E': '%s'", p.error.c_str());
    }
    {  // F: mask_l has bits below 16
        Call c = one_file(1 * MiB);
        c.mn = 64, c.av = 1024, c.mx = 2048;
        expect("F", c, false, 524288, -1, 512, 8226, 2);
        c.walk_env = 1;
        expect_error("F'", c, "masks below bit 16 or an unaligned arena");
        oxh::CdcPlan p;
        run(c, p);
        CHECK(p.error == "OXH_CDC_WALK=1: masks below bit 16 or an unaligned arena", "F': '%s'", p.error.c_str());
    }
    {  // G: a section override below max is raised to it
        Call c = B;
        c.sec_env = 1024;
        expect("G", c, true, 16384, 32768, 8, 10, 64);
    }
    {  // H: every override at once
        Call c = B;
        c.walk_env = 0, c.sec_env = 16384, c.cap_env = 1, c.warmup_env = 0;
        expect("H", c, false, 16384, 0, 1, 10, 64);
    }
    {  // I: empty files own no section
        Call c = B;
        c.off = {0, 0, 256};
        c.len = {0, 1, 0};
        expect("I", c, true, 65536, 32768, 10, 22, 1, {0, 0, 1, 1});
    }
    {  // J: sections grow so that one generation of waves covers the input: whole 8 KiB above
       // ceil(total / (256 CUs * 12 waves * 64 lanes))
        Call c = one_file(16 * GiB);
        expect("J", c, true, 90112, 32768, -1, 28, 190651);
    }
    {  // K: the boundary of the default choice
        Call c = one_file(1 * MiB);
        c.mn = 4096, c.av = 16384, c.mx = 32768;
        oxh::CdcPlan p;
        CHECK(run(c, p) == OXH_OK && p.walk, "K: avg 16384 plans %s", p.walk ? "walk" : "scan");
        c.av = 16385;
        CHECK(run(c, p) == OXH_OK && !p.walk, "K: avg 16385 plans %s", p.walk ? "walk" : "scan");
    }
    {  // no file at all: an empty table
        Call c = B;
        c.off.clear(), c.len.clear();
        expect("empty", c, true, 65536, 32768, 10, 22, 0, {0});
    }
}

void param_checks() {
    const char* msg = nullptr;
    CHECK(oxh::cdc_check_params(4096, 8192, 16384, 1, &msg) == OXH_OK && msg == nullptr, "valid sizes refused");
    struct Bad {
        uint32_t mn, av, mx, lv;
        const char* text;
    } bad[] = {
        {63, 8192, 16384, 1, "min_size must be in [64, 1048576]"},
        {1048577, 8192, 16384, 1, "min_size must be in [64, 1048576]"},
        {4096, 255, 16384, 1, "avg_size must be in [256, 4194304]"},
        {4096, 4194305, 16384, 1, "avg_size must be in [256, 4194304]"},
        {4096, 8192, 1023, 1, "max_size must be in [1024, 16777216]"},
        {4096, 8192, 16777217, 1, "max_size must be in [1024, 16777216]"},
        {4096, 8192, 16384, 4, "normalization level must be 0..3"},
    };
    for (const Bad& b : bad) {
        CHECK(oxh::cdc_check_params(b.mn, b.av, b.mx, b.lv, &msg) == OXH_ERR_INVALID && msg && !strcmp(msg, b.text),
              "%u/%u/%u/%u: '%s'", b.mn, b.av, b.mx, b.lv, msg ? msg : "(none)");
        Call c = one_file(1 * MiB);
        c.mn = b.mn, c.av = b.av, c.mx = b.mx, c.lv = b.lv;
        expect_error("bad sizes", c, b.text);
    }
    for (uint32_t v : {64u, 1048576u}) CHECK(oxh::cdc_check_params(v, 8192, 16384, 0, &msg) == OXH_OK, "min %u", v);
    // fastcdc v2020: MASKS[13 +/- 1] at avg 8192, level 1
    uint64_t ms = 0, ml = 0;
    oxh::cdc_masks(8192, 1, &ms, &ml);
    CHECK(ms == 0x0000d90313530000ULL && ml == 0x0000d90103530000ULL, "masks %" PRIx64 " %" PRIx64, ms, ml);
    CHECK(oxh::log2_round(256) == 8 && oxh::log2_round(4194304) == 22 && oxh::log2_round(11585) == 13 &&
              oxh::log2_round(11586) == 14,
          "log2_round");
}

// the window rule as the planner states it: a wave's lowest start (warm-up included) to the highest
// byte one of its lanes may read, from a 128-B line, within 4 GiB - 1 MiB
bool windows_hold(const Call& c, const oxh::CdcPlan& p) {
    const oxh::CdcParams& prm = p.prm;
    for (uint64_t w0 = 0; w0 < p.n_sec; w0 += 64) {
        uint64_t lo = ~0ull, hi = 0;
        for (uint64_t s = w0; s < p.n_sec && s < w0 + 64; ++s) {
            size_t f = 0;
            while (p.sec_base[f + 1] <= s) ++f;
            const uint64_t ss = (s - p.sec_base[f]) * prm.sec;
            const uint64_t a = c.off[f] + (ss > prm.warmup ? ss - prm.warmup : 0);
            const uint64_t e = ss + prm.sec + 2 * prm.max + 4096;
            const uint64_t b = c.off[f] + (c.len[f] < e ? c.len[f] : e);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        if (hi - (lo & ~127ull) + 256 >= 0xFFFFFF00ull - (1ull << 20)) return false;
    }
    return true;
}

void invariants() {
    for (uint32_t av : {256u, 1024u, 4096u, 8192u, 16384u, 65536u, 4194304u})
        for (uint32_t lv = 0; lv <= 3; ++lv) {
            Call c = one_file(1);
            c.av = av, c.lv = lv;
            // min = max(64, avg / 2), held to the crate's upper bound for min at the largest avg
            c.mn = av / 2 < 64 ? 64 : av / 2 > 1048576 ? 1048576 : av / 2;
            c.mx = 2 * av < 1024 ? 1024 : 2 * av;
            oxh::CdcPlan p0;
            int rc = run(c, p0);
            CHECK(rc == OXH_OK, "avg %u level %u: rc %d (%s)", av, lv, rc, p0.error.c_str());
            if (rc != OXH_OK) continue;
            const uint64_t sec = p0.prm.sec;
            c.len = {0, 1, sec - 1, sec, sec + 1};
            c.off.clear();
            uint64_t at = 0;
            for (uint64_t l : c.len) {
                c.off.push_back(at);
                at = (at + l + 255) & ~255ull;
            }
            oxh::CdcPlan p;
            rc = run(c, p);
            CHECK(rc == OXH_OK, "avg %u level %u: rc %d (%s)", av, lv, rc, p.error.c_str());
            if (rc != OXH_OK) continue;
            const oxh::CdcParams& prm = p.prm;
            const uint64_t max_rounded = ((uint64_t)c.mx + 1023) / 1024 * 1024;
            CHECK(prm.sec == sec, "avg %u level %u: sec %" PRIu64 " then %" PRIu64, av, lv, sec, prm.sec);
            CHECK(prm.sec % 8192 == 0, "avg %u level %u: sec %" PRIu64, av, lv, prm.sec);
            CHECK(max_rounded <= prm.sec && prm.sec <= 128 * MiB, "avg %u level %u: sec %" PRIu64, av, lv, prm.sec);
            CHECK(prm.unit == prm.sec / 64, "avg %u level %u: unit %" PRIu64, av, lv, prm.unit);
            CHECK(1 <= prm.cap && prm.cap <= prm.unit / 16, "avg %u level %u: cap %u of unit %" PRIu64, av, lv, prm.cap,
                  prm.unit);
            CHECK(p.sec_base.size() == c.len.size() + 1 && p.sec_base[0] == 0, "avg %u level %u: sec_base", av, lv);
            for (size_t i = 0; i + 1 < p.sec_base.size(); ++i)
                CHECK(p.sec_base[i + 1] - p.sec_base[i] == (c.len[i] + prm.sec - 1) / prm.sec,
                      "avg %u level %u: file %zu of %" PRIu64 " B has %" PRIu64 " sections", av, lv, i, c.len[i],
                      p.sec_base[i + 1] - p.sec_base[i]);
            CHECK(p.n_sec == p.sec_base.back() && p.n_sec == 5, "avg %u level %u: n_sec %" PRIu64, av, lv, p.n_sec);
            CHECK(p.total_bytes == 3 * sec + 1 && p.arena_bytes == c.off.back() + c.len.back(),
                  "avg %u level %u: totals %" PRIu64 " %" PRIu64, av, lv, p.total_bytes, p.arena_bytes);
            if (p.walk) {
                CHECK(2 * (uint64_t)prm.speccap * 4 + 2048 <= (uint64_t)kLds, "avg %u level %u: speccap %u", av, lv,
                      prm.speccap);
                CHECK(windows_hold(c, p), "avg %u level %u: a wave's window", av, lv);
                CHECK(((prm.mask_s | prm.mask_l) & 0xFFFF) == 0, "avg %u level %u: masks", av, lv);
            }
        }
}

}  // namespace

int main() {
    table();
    param_checks();
    invariants();
    if (g_failed) {
        fprintf(stderr, "cdc_plan_test: %d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("cdc_plan_test: all %d checks passed\n", g_checks);
    return 0;
}
