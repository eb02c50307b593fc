// oxen_amd/csrc/fastcdc_plan.hpp -- the host arithmetic of one oxh_fastcdc_device call: the crate's
// parameter checks, the mask selection, and the section plan (scan or walk, section size, warm-up,
// list capacities, the per-file section table). Pure integer work on host values: no HIP header and
// no environment read (the caller passes the device facts and the env.hpp overrides in), so
// tests/native/cdc_plan_test.cpp exercises it with plain g++ on any host.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/oxen_hash.h"

namespace oxh {

// fastcdc::v2020::MASKS, indexed by the number of one bits (entries 0..4 are padding)
static constexpr uint64_t kCdcMasks[26] = {
    0, 0, 0, 0, 0,
    0x0000000001804110ULL, 0x0000000001803110ULL, 0x0000000018035100ULL, 0x0000001800035300ULL,
    0x0000019000353000ULL, 0x0000590003530000ULL, 0x0000d90003530000ULL, 0x0000d90103530000ULL,
    0x0000d90303530000ULL, 0x0000d90313530000ULL, 0x0000d90f03530000ULL, 0x0000d90303537000ULL,
    0x0000d90703537000ULL, 0x0000d90707537000ULL, 0x0000d91707537000ULL, 0x0000d91747537000ULL,
    0x0000d91767537000ULL, 0x0000d93767537000ULL, 0x0000d93777537000ULL, 0x0000d93777577000ULL,
    0x0000db3777577000ULL,
};

constexpr uint32_t kSecDefault = 512 * 1024;  // minimum section bytes (F1 wave / F2 lane unit)
constexpr int kScanWaves = 12;                // waves per F1 / W workgroup (fastcdc_scan.hip has the reasons)
constexpr uint64_t kXStaticLds = 256 * 8;     // the X kernels' static LDS (their gear table), beside the dynamic lists

struct CdcParams {
    uint64_t min, avg, max;
    uint64_t mask_s, mask_l;
    uint64_t sec;      // section bytes: a multiple of 8 KiB (F1 wave / F2 lane unit)
    uint64_t unit;     // sec / 64: the candidate list unit (F1 lane)
    uint64_t warmup;   // bytes a speculative walk runs before its section (unrecorded)
    uint32_t cap;      // candidate entries stored per unit
    uint32_t speccap;  // speculative chunk starts stored per section
};

// v2020::FastCDC::with_level asserts (crate fastcdc 3.2.1): OXH_OK, or OXH_ERR_INVALID and its text
inline int cdc_check_params(uint32_t min_size, uint32_t avg_size, uint32_t max_size, uint32_t level, const char** msg) {
    *msg = nullptr;
    if (min_size < 64 || min_size > 1048576) *msg = "min_size must be in [64, 1048576]";
    else if (avg_size < 256 || avg_size > 4194304) *msg = "avg_size must be in [256, 4194304]";
    else if (max_size < 1024 || max_size > 16777216) *msg = "max_size must be in [1024, 16777216]";
    else if (level > 3) *msg = "normalization level must be 0..3";
    return *msg ? OXH_ERR_INVALID : OXH_OK;
}

inline uint32_t log2_round(uint32_t v) {
    const uint32_t b = 31 - (uint32_t)__builtin_clz(v);
    const double x = (double)v, lo = (double)(1u << b);
    return (x * x >= 2.0 * lo * lo) ? b + 1 : b;
}

// MASKS[bits +/- level], bits = round(log2(avg)); avg and level within cdc_check_params' ranges
inline void cdc_masks(uint32_t avg_size, uint32_t level, uint64_t* mask_s, uint64_t* mask_l) {
    const uint32_t bits = log2_round(avg_size);
    *mask_s = kCdcMasks[bits + level];
    *mask_l = kCdcMasks[bits - level];
}

struct CdcPlanInput {
    const uint64_t* offsets;  // [n] arena offset of each file
    const uint64_t* lens;     // [n]
    uint64_t n;
    uint32_t min_size, avg_size, max_size, level;
    uint64_t arena_addr;      // the arena's device address (its low 7 bits: the walk wants 128-B alignment)
    int cus, max_lds;         // the device: compute units, and the most LDS one workgroup may have
    // the env.hpp overrides, as their readers return them (-1 = unset): cdc_walk(), cdc_section_bytes(),
    // cdc_warmup_bytes(), cdc_unit_cap()
    int walk_env;
    long long sec_env, warmup_env;
    int cap_env;
};

struct CdcPlan {
    CdcParams prm;
    bool walk;                       // W + X; otherwise the scan F1-F3
    std::vector<uint64_t> sec_base;  // [n+1] first global section of each file
    uint64_t n_sec, total_bytes, arena_bytes;
    std::string error;               // set with a non-zero return
};

inline int cdc_plan(const CdcPlanInput& in, CdcPlan& out) {
    const char* bad = nullptr;
    if (int rc = cdc_check_params(in.min_size, in.avg_size, in.max_size, in.level, &bad)) {
        out.error = bad;
        return rc;
    }
    auto fail = [&](const std::string& msg) {
        out.error = msg;
        return (int)OXH_ERR_INVALID;
    };
    const uint64_t n = in.n;
    const uint32_t min_size = in.min_size, max_size = in.max_size;
    CdcParams& prm = out.prm;
    prm = CdcParams{};
    prm.min = min_size;
    prm.avg = in.avg_size;
    prm.max = max_size;
    cdc_masks(in.avg_size, in.level, &prm.mask_s, &prm.mask_l);
    // F1 records a 16-byte group wherever the bits both masks share are clear at one of its bytes:
    // ~16 * 2^-popcount(common) groups per 16 bytes. Store 8x the expected count (+8) per list unit
    // (sec / 64 bytes), at most one per group; a denser unit keeps a truncated list and the walk
    // scans its bytes (C5 at 8 KiB: 2 expected per 8 KiB unit, 24 stored: P(overflow) ~ 1e-16).
    const double dens = std::min(1.0, 16.0 * std::ldexp(1.0, -__builtin_popcountll(prm.mask_s & prm.mask_l))) / 16.0;
    // sections of at least `max` bytes: a chunk never spans a whole section (F3's invariant)
    // Speculative walks meet the true walk after ~1.5 chunks (median) and within 6 chunks in 99 % of
    // random starts (measured with the oracle). Warm-up: 6 max-sized chunks, at least 128 KiB (r02
    // sweep, walk + fixup: 64 KiB chunks 2.57 / 2.09 / 2.18 ms at 512 / 768 / 1024 KiB; 8 KiB chunks
    // 3.95 / 3.89 / 4.06 / 4.43 ms at 96 / 128 / 192 / 256 KiB);
    // sections: at least 8 max-sized chunks and 512 KiB. Every section whose walk has not met the
    // true one is re-walked serially by F3, so at small chunk sizes the longer warm-up pays for itself
    // (C5 at 8 KiB: 57.2 ms vs 63.8 ms with 256 KiB sections and 64 KiB of warm-up; at 64 KiB: 53.8
    // vs 54.9 ms with 1 MiB sections; tools/bench_fastcdc.py sweeps).
    const uint64_t max_rounded = ((uint64_t)max_size + 1023) / 1024 * 1024;
    out.total_bytes = out.arena_bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        out.total_bytes += in.lens[i];
        out.arena_bytes = std::max<uint64_t>(out.arena_bytes, in.offsets[i] + in.lens[i]);
    }
    // The walk path (W + X, DESIGN §4 "F1 -> W"): chosen where it rolls fewer bytes than F1 -- small
    // chunks, where the skipped `min` bytes are a large share (61 % rolled at 8 KiB, 94 % at 64 KiB) --
    // and where its layout rules hold: masks at bit 16 or above, a 128-B aligned arena, every wave's 64
    // sections inside one 4 GiB window, and X's per-section lists within a workgroup's LDS (checked
    // below; where one does not hold the call takes the scan). OXH_CDC_WALK=0 / 1 forces it off / on.
    const bool walk_forced = in.walk_env == 1;
    bool walk = (((prm.mask_s | prm.mask_l) & 0xFFFFull) == 0) && ((in.arena_addr & 127) == 0) &&
                (in.walk_env >= 0 ? walk_forced : (in.avg_size <= 16384));
    if (walk_forced && !walk) return fail("OXH_CDC_WALK=1: masks below bit 16 or an unaligned arena");
    const long long sec_env = in.sec_env;  // tests: many small sections per file
    std::vector<uint64_t>& sec_base = out.sec_base;
    sec_base.assign(n + 1, 0);
    for (;;) {
        prm.sec = kSecDefault;
        if (sec_env >= 1024 && sec_env % 1024 == 0 && sec_env <= (1 << 30)) prm.sec = (uint64_t)sec_env;
        prm.warmup = std::max<uint64_t>(6 * (uint64_t)max_size, 128 * 1024);
        if (walk) {
            // one lane per section, one generation of 12-wave workgroups on every CU: sections as large
            // as that allows (fewer sections = less warm-up and stitching), whole 8 KiB, at least 4 max
            const uint64_t lanes = (uint64_t)in.cus * kScanWaves * 64;
            const uint64_t want = (out.total_bytes + lanes - 1) / std::max<uint64_t>(lanes, 1);
            if (sec_env < 0) prm.sec = std::max<uint64_t>({want, 4 * max_rounded, 64 * 1024});
            // warm-up: a relaxed walk started anywhere lands on the true one within 14 / 37 / 67 KB in 50 /
            // 90 / 99 % of starts at 8 KiB chunks (C restatement, 1 GiB); X re-walks the sections whose
            // warm-up was too short, so it is kept short: two max-sized chunks
            prm.warmup = 2 * (uint64_t)max_size;
        }
        if (prm.sec < max_rounded) prm.sec = max_rounded;
        if (!walk && sec_env < 0 && prm.sec < 8 * max_rounded) prm.sec = 8 * max_rounded;
        prm.sec = (prm.sec + 8191) / 8192 * 8192;  // 64 F1 units of whole 128-byte rounds
        // a candidate entry holds the group index in 17 bits: units of at most 2 MiB (sections of 128 MiB,
        // 8 chunks of the crate's largest max); the test-only section override is clamped to that
        prm.sec = std::min<uint64_t>(prm.sec, 128ull << 20);
        // (still >= max_rounded: sec was raised to it above, and max_rounded is at most 16 MiB)
        prm.unit = prm.sec / 64;
        if (in.warmup_env >= 0) prm.warmup = (uint64_t)in.warmup_env;  // tests
        prm.cap = (uint32_t)std::min<double>(prm.unit / 16, 8.0 * dens * prm.unit + 8);
        if (in.cap_env > 0) prm.cap = (uint32_t)in.cap_env;  // tests: force overflow
        prm.speccap = (uint32_t)(prm.sec / min_size + 2 + (max_size + min_size - 1) / min_size);

        sec_base[0] = 0;
        for (uint64_t i = 0; i < n; ++i) sec_base[i + 1] = sec_base[i] + (in.lens[i] + prm.sec - 1) / prm.sec;
        out.n_sec = sec_base[n];
        if (!walk) break;
        // X keeps a section's start list and fix list in dynamic LDS beside its static gear table
        std::string why;
        if (2 * (uint64_t)prm.speccap * sizeof(uint32_t) + kXStaticLds > (uint64_t)in.max_lds)
            why = "X's section lists do not fit the workgroup's LDS";
        // every wave's lanes must address their streams from one buffer resource: the lowest start
        // (warm-up included) to the highest byte a lane may read (its section end + two max chunks,
        // or its file end) within 4 GiB - 1 MiB
        for (uint64_t w0s = 0, f = 0; w0s < out.n_sec && why.empty(); w0s += 64) {
            uint64_t lo = ~0ull, hi = 0;
            for (uint64_t sct = w0s; sct < std::min<uint64_t>(out.n_sec, w0s + 64); ++sct) {
                while (sec_base[f + 1] <= sct) ++f;
                const uint64_t ss = (sct - sec_base[f]) * prm.sec;
                const uint64_t a = in.offsets[f] + (ss > prm.warmup ? ss - prm.warmup : 0);
                const uint64_t b = in.offsets[f] + std::min<uint64_t>(in.lens[f], ss + prm.sec + 2 * prm.max + 4096);
                lo = std::min(lo, a);
                hi = std::max(hi, b);
            }
            if (hi - (lo & ~127ull) + 256 >= 0xFFFFFF00ull - (1ull << 20)) why = "a wave's sections span 4 GiB";
        }
        if (why.empty()) break;
        if (walk_forced) return fail("OXH_CDC_WALK=1: " + why);
        walk = false;  // the scan, with its own section plan
    }
    out.walk = walk;
    return OXH_OK;
}

}  // namespace oxh
