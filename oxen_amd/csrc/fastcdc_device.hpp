// oxen_amd/csrc/fastcdc_device.hpp -- what the FastCDC translation units share on the device:
// fastcdc_scan.hip (F1-F3), fastcdc_walk.hip (W + X) and fastcdc.hip (the kernels after either, and
// the C entries). The tables both pipelines read and write, the small device helpers, and cut_gear's
// window arithmetic (cut_window), which has to match the crate exactly and so exists once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fastcdc_gear.h"
#include "fastcdc_plan.hpp"

namespace oxh {

constexpr int kHashSpan = 47;          // positions after a chunk's start index with a truncated window
constexpr int kEntryShift = 47;        // candidate entry: group index (17 bits: units up to 2 MiB) << 47 | hash
constexpr uint64_t kEntryHash = (1ull << kEntryShift) - 1;
constexpr int kScanDmaAux = 2;  // cache policy of the scan's and the walk's LDS-DMA loads (2 = nt)

// One recorded candidate group: its entry (group index in the unit << 47 | the full-window hash
// before its first byte mod 2^47; bit 47 and up never reach a masked bit once the walk shifts it, so
// 47 bits suffice) and its 16 bytes (the walk resolves exact flags from these), in one 32-byte record:
// F1's two stores and the walk's two loads of a candidate touch one cache line, not one in each of
// two arrays.
// The first record of a unit's list also carries the unit's true candidate count in `n` (> cap: the
// list was truncated and the walk scans the rest of the unit's bytes), so a walk entering a unit
// gets the count and the first candidate from one line.
struct alignas(16) CandRec {
    uint64_t e;
    uint64_t n;  // record 0 of a unit: the unit's count; unused in the others
    uint4 b;
};

struct CdcFiles {
    const uint8_t* arena;
    const uint64_t* foff;      // [n] arena offset of each file
    const uint64_t* flen;      // [n]
    const uint64_t* sec_base;  // [n+1] first global section of each file
    const uint32_t* sec_file;  // [n_sec] file of each section
    CandRec* cand;             // [n_sec * 64 * cap] candidate groups per unit, in position order
    uint64_t* cand_occ;        // [n_sec] bit u: unit u of the section has a non-empty list
    uint32_t* spec;            // [n_sec * speccap] speculative starts, relative to section start
    uint32_t* spec_cnt;        // [n_sec]
};

// The stitch tables (fastcdc_scan.hip "F3" has the argument; X fills the same tables for the walk).
enum : uint32_t { kConverged = 0, kFailed = 1, kFixed = 2 };

struct CdcStitch {
    uint32_t* status;   // [n_sec]
    uint32_t* k0;       // [n_sec] first speculative entry of the true walk (converged)
    uint32_t* count;    // [n_sec] true starts inside the section
    uint64_t* exit;     // [n_sec] file-relative entry of the next section (or the file length)
    uint32_t* fix;      // [n_sec * speccap] re-walked starts, relative to the section start
    uint64_t* out_base; // [n_sec + 1] exclusive prefix of count (global chunk index)
};

// The two pipelines, each launched on `st` up to (not including) the prefix sum: the first launch
// error, if any. fastcdc_scan.hip: F1, F2, F3a, F3b. fastcdc_walk.hip: W, X, X-retry, X-fix.
hipError_t cdc_launch_scan(const CdcFiles& f, const CdcParams& prm, const CdcStitch& s, uint64_t n_sec, uint64_t n_files,
                           hipStream_t st);
hipError_t cdc_launch_walk(const CdcFiles& f, const CdcParams& prm, const CdcStitch& s, uint64_t n_sec, uint64_t n_files,
                           uint64_t arena_bytes, uint32_t* d_entry, hipStream_t st);

__device__ __forceinline__ uint64_t gear_of(const uint64_t* __restrict__ g, uint32_t b) { return g[b]; }

// DPP wave_shr:1 (GFX9): lane l gets x from lane l-1; lane 0 keeps `old`
__device__ __forceinline__ uint32_t wave_shr1(uint32_t x, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)x, 0x138, 0xf, 0xf, false);
}
// (a & b) | c in one VALU op
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
// min of three: the backend forms v_min3_u32 from the nested umin. (An inline-asm v_min3 made the
// compiler put an `s_nop 0` between every two asm blocks -- it cannot see their hazards -- one wasted
// issue slot per 4 bytes in F1, ~5 % of its issue-bound loop.)
__device__ __forceinline__ uint32_t min3_u32(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_elementwise_min(__builtin_elementwise_min(a, b), c);
}

// 16 bytes at p[pos .. pos+16) of a file of length flen as four little-endian words (zeros past the
// end): one unaligned global_load_dwordx4 (gfx950 runs in unaligned-access mode) instead of 16
// dependent byte loads -- the walk's latency is made of these. Not a buffer load: every lane of the
// walk has its own address, and a buffer resource built from a per-lane pointer is not wave-uniform,
// so the compiler wrapped each such load in a readfirstlane loop that issued it once per lane (64x;
// the walk took 3.7 ms of C5 at 8 KiB chunks with it).
__device__ __forceinline__ uint4 load16_file(const uint8_t* __restrict__ fbase, uint64_t pos, uint64_t flen) {
    if (pos >= flen) return make_uint4(0, 0, 0, 0);
    if (flen - pos >= 16) {
        typedef unsigned int u32x4u __attribute__((ext_vector_type(4), aligned(1)));
        const u32x4u v = *(const u32x4u*)(fbase + pos);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (pos + (uint64_t)j < flen) w[j >> 2] |= (uint32_t)fbase[pos + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint32_t byte_of(const uint4& v, int j) {
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 0xFF;
}

// cut_gear's window (crate fastcdc 3.2.1, v2020) for a chunk with `len` bytes left from its start.
// cut_whole: len <= min, the chunk is everything left and nothing is hashed. Otherwise cut_window: the
// hash starts from 0 at index a0, positions [a0, eS) test mask_s, [eS, eL) test mask_l, and the chunk
// is `rem` bytes when none matches. (W's walk_begin_chunk restates this in 32 bits: fastcdc_walk.hip
// says why.)
struct CutWindow {
    uint64_t rem, a0, eS, eL;
};
__device__ __forceinline__ bool cut_whole(uint64_t len, const CdcParams& prm) { return len <= prm.min; }
__device__ __forceinline__ CutWindow cut_window(uint64_t len, const CdcParams& prm) {
    const uint64_t rem = len > prm.max ? prm.max : len;
    uint64_t center = prm.avg;
    if (len <= prm.max && len < center) center = len;
    return {rem, prm.min & ~1ull, center & ~1ull, rem & ~1ull};
}

}  // namespace oxh
