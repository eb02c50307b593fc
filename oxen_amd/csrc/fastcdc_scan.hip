// oxen_amd/csrc/fastcdc_scan.hip -- FastCDC's scan pipeline (F1-F3) on gfx950: taken for avg > 16 KiB
// and wherever the walk's layout rules fail (fastcdc_plan.hpp chooses; fastcdc.hip has the overview).
//
// The walk is serial per file (each cut decides where the next chunk's hash starts). The GPU
// formulation splits it into three kernels:
//   F1 cdc_scan_kernel    chip-wide, one wave per section (>= 512 KiB), lane-major: lane l rolls
//                         the gear hash through unit l (section / 64 bytes) from 48 bytes before it,
//                         so it has the FULL-window hash at every byte (all mask bits are below bit
//                         48: the hash of position p is a function of b[p-47 .. p]), and records a
//                         position-ordered list of candidate 16-byte groups per unit (a position with
//                         none of the bits both masks share clear).
//   F2 cdc_walk_kernel    one lane per section: a speculative walk that starts 6 max-sized chunks
//                         before the section (by then it has almost surely met the true walk) and
//                         cuts chunks from the candidate lists until it passes the section end,
//                         recording the starts inside the section. The first 47 positions after a chunk's `min` see a hash
//                         that started from 0 (truncated window); the walk recomputes those from the
//                         bytes, everything later comes from the candidates.
//   F3 stitch             cdc_check_kernel (one lane per section): the last start section i-1's
//                         walk recorded is the true entry of section i; if section i's own walk
//                         produced that start too, the rest of its list is the true walk (cut
//                         points depend only on the chunk start). cdc_fixup_kernel re-walks the
//                         sections where that failed; a prefix sum and cdc_emit_kernel (fastcdc.hip)
//                         write the chunk table.
#include "fastcdc_device.hpp"

namespace oxh {

// ---------------------------------------------------------------- F1: candidates
// Lane-major scan. A section of S bytes is split into 64 list units of U = S/64 bytes; lane l owns
// unit l and rolls ONE hash through it, starting from the 48 bytes before the unit (warm-up; only
// the last 48 bytes reach the masked bits, so the rolled hash is the full-window hash from the unit's
// first byte on). Per byte: one v_perm_b32 (the LDS address: byte << 8 | copy offset), one
// ds_read_b64, one v_lshl_add_u64, one AND and a share of a v_min3 -- against ~6.4 VALU per byte for
// the wave-cooperative form this replaces, which rolled every byte twice (the lane-local hash, then
// again from the carry of the three lanes before it).
//
// The bytes reach the lanes through LDS without a VGPR round trip: a round is 128 B of every unit;
// 8 `buffer_load_dwordx4 ... lds` per round (lanes 8m..8m+7 of DMA k fetch the whole 128-B line of
// unit 8k+m, so every line is fetched once, coalesced) land unit r's bytes at slot + 128 r, and lane
// r reads them back with 8 ds_read_b128. The DMA lanes fetch their pieces rotated (piece q of unit r
// at position (q + (r >> 1)) & 7 of its line) so that the 16 lanes of every ds_read_b128 group cover
// the 64 banks exactly once. The gear table is stored 32 times (entry k of copy c at byte 256 k + 8 c,
// lane l reads copy l % 32): the 32 lanes of a ds_read_b64 group never share a bank.
// LDS: 64 KiB table + one 8 KiB slot per wave (the round being rolled sits in VGPRs while the next
// round's DMA is in flight): 160 KiB at 12 waves per workgroup. tools/cdc_segment_probe.hip has the variants this was chosen from.
//
// Candidates: a lane records a 16-byte group of its unit when one of its positions has none of the
// bits both masks share (offset in the unit, the hash before the group, its 16 bytes); the walk
// resolves exact mask_s / mask_l flags from those. Lists are per unit, in position order.
//
// SH: the whole hash runs 16 bits to the left (table entries GEAR << 16, masks << 16; only bits below
// 48 matter). When the bits both masks share are all >= 16 they then sit in the high 32-bit word and
// the per-byte test is one AND; otherwise (avg < ~2 KiB) the low word is tested too (v_and_or).
// 12 waves per workgroup (kScanWaves): the 64 KiB table + 12 x 8 KiB slots fill the 160 KiB of LDS, 3 waves per
// SIMD (119 VGPRs) instead of 2. The roll is one dependent v_lshl_add_u64 chain per lane, so the
// third wave's chain fills issue slots (C5 at 8 KiB: F1 26.6 vs 28.2 ms with 8 waves, r02). 16 waves
// with 64-byte rounds (4 KiB slots, half-line DMA) measured far slower (73 vs 52 ms end to end).
template <bool SH>
__global__ __launch_bounds__(64 * kScanWaves) void cdc_scan_kernel(CdcFiles f, CdcParams prm, uint64_t n_sec) {
    // one LDS block: the table at address 0 (a gather address is then a single v_perm), slots after it
    __shared__ __attribute__((aligned(16))) uint64_t lds[256 * 32 + kScanWaves * 1024];
    for (int i = threadIdx.x; i < 256 * 32; i += blockDim.x) lds[i] = kGear[i >> 5] << (SH ? 16 : 0);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint4* const slot = (uint4*)(lds + 256 * 32) + w * 512;
    const uint64_t sec = (uint64_t)blockIdx.x * kScanWaves + (uint64_t)w;
    if (sec >= n_sec) return;
    const uint32_t file = f.sec_file[sec];
    const uint64_t flen = f.flen[file];
    const uint64_t sec_start = (sec - f.sec_base[file]) * prm.sec;
    const uint32_t sec_len = (uint32_t)(flen - sec_start < prm.sec ? flen - sec_start : prm.sec);
    const uint8_t* __restrict__ base = f.arena + f.foff[file] + sec_start;
    const uint32_t unit = (uint32_t)prm.unit, rounds = unit / 128;
    const uint32_t us = (uint32_t)lane * unit;  // this lane's unit, section-relative
    // the resource covers the 48 bytes before the section (none at a file start) and every whole
    // 16-byte piece of the section: loads past it return zeros without touching memory
    const uint32_t pre = sec_start > 0 ? 48u : 0u, full16 = sec_len & ~15u;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)(base - pre), (short)0, (int)(pre + full16), 0x00020000);
    const uint64_t mask_s = prm.mask_s << (SH ? 16 : 0), mask_l = prm.mask_l << (SH ? 16 : 0);
    const uint64_t common = mask_s & mask_l;
    const uint32_t ch = (uint32_t)(common >> 32), cl = (uint32_t)common;  // SH: cl == 0 (host checks)
    const uint32_t copy_off = (uint32_t)(lane & 31) * 8;
    const char* const tab = (const char*)lds;
    auto gear = [&](uint32_t word, int j) -> uint64_t {
        const uint32_t a = __builtin_amdgcn_perm(word, copy_off, 0x0c0c0000u | ((4u + (uint32_t)j) << 8));
        return *(const uint64_t*)(tab + a);
    };
    const uint64_t ubase = sec * 64 + (uint64_t)lane;  // global unit index
    CandRec* __restrict__ out_c = f.cand + ubase * prm.cap;
    uint32_t count = 0;  // per lane

    // warm-up over the 48 bytes before the unit (lane 0 at a file start: none, the hash starts at 0)
    uint64_t h = 0;
    {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        uint32_t wv[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, pre + us - 48 + 16 * k, 0, 0);
            wv[4 * k] = v.x, wv[4 * k + 1] = v.y, wv[4 * k + 2] = v.z, wv[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) h = (h << 1) + gear(wv[i], b);
        if (pre + us < 48) h = 0;
    }
    // round t of every unit into this wave's slot (DMA k, lane 8m + j: unit 8k + m, rotated piece)
    const int dm = lane >> 3, dj = lane & 7;
    // the round moves the resource (SGPR arithmetic: its base by 128 B, its size down by as much) rather
    // than the 8 per-lane offsets (8 VALU adds per round); the whole offset stays in the VGPR operand,
    // so the range check sees it: a piece at or past the section's last whole 16 bytes reads zeros
    uint32_t voff[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t r = 8 * k + dm;
        voff[k] = pre + r * unit + 16 * ((uint32_t)(dj - (int)((r >> 1) & 7)) & 7);
    }
    auto dma_round = [&](uint32_t t) {
        // wave-uniform by construction; readfirstlane keeps the compiler from treating the resource
        // as per-lane (which would wrap every DMA in a readfirstlane loop)
        const int left = __builtin_amdgcn_readfirstlane((int)(pre + full16 > t * 128 ? pre + full16 - t * 128 : 0u));
        const uint64_t a = (uint64_t)(base - pre) + (uint64_t)t * 128;
        const uint64_t au = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32);
        const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc((void*)au, (short)0, left, 0x00020000);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rt, (__attribute__((address_space(3))) void*)(slot + 64 * k), 16, voff[k],
                                                     0, 0, kScanDmaAux);
    };
    dma_round(0);
    const int rot = (lane >> 1) & 7;
    // the round (if any) whose 128 B hold the section's partial last 16 bytes, for this lane
    const uint32_t t_part = (sec_len != full16 && us <= full16 && full16 < us + unit) ? (full16 - us) >> 7 : 0xFFFFFFFFu;
#pragma unroll 1
    for (uint32_t t = 0; t < rounds; ++t) {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this round's DMA has landed
        uint32_t wv[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint4 v = slot[lane * 8 + ((q + rot) & 7)];
            wv[4 * q] = v.x, wv[4 * q + 1] = v.y, wv[4 * q + 2] = v.z, wv[4 * q + 3] = v.w;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the slot is free for the next DMA
        if (t + 1 < rounds) dma_round(t + 1);
        const uint32_t rb = us + t * 128;  // section-relative start of this lane's 128 B
        // the section's partial last 16 B (outside the resource): byte loads, in the one lane that has it
        if (t == t_part) {
            const int pi = (int)((full16 - rb) >> 4);
            uint32_t pw[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t q = 0; q < 16; ++q)
                if (full16 + q < sec_len) pw[q >> 2] |= (uint32_t)base[full16 + q] << (8 * (q & 3));
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q == pi) wv[4 * q] = pw[0], wv[4 * q + 1] = pw[1], wv[4 * q + 2] = pw[2], wv[4 * q + 3] = pw[3];
        }
        // roll the 128 bytes; the gathers of word i + P are issued before word i is rolled
        constexpr int P = 3;
        uint64_t G[P + 1][4];
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) G[i][b] = gear(wv[i], b);
        uint64_t hb = h;  // the hash before the current group
        // opaque copy: kept in two VGPRs (otherwise hipcc may re-derive it inside the rare record
        // branch from the rolled hashes, which costs hundreds of extra shift-adds per round)
        asm volatile("" : "+v"(hb));
        uint32_t anyz = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if (i + P < 32) {
#pragma unroll
                for (int b = 0; b < 4; ++b) G[(i + P) % (P + 1)][b] = gear(wv[i + P], b);
            }
            __builtin_amdgcn_sched_barrier(0);
            uint32_t tt[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                h = (h << 1) + G[i % (P + 1)][b];
                if constexpr (SH) tt[b] = (uint32_t)(h >> 32) & ch;
                else tt[b] = ((uint32_t)h & cl) | ((uint32_t)(h >> 32) & ch);
            }
            anyz = min3_u32(min3_u32(anyz, tt[0], tt[1]), tt[2], tt[3]);  // two v_min3 per 4 bytes
            if ((i & 3) == 3) {
                // one VALU compare and a uniform branch when no lane of the wave has a candidate here
                if (__builtin_amdgcn_ballot_w64(anyz == 0)) {
                    const uint32_t g = rb + 16 * (uint32_t)(i >> 2);  // the group, section-relative
                    if (anyz == 0 && g < sec_len) {
                        if (count < prm.cap) {
                            out_c[count].e = ((uint64_t)((g - us) >> 4) << kEntryShift) | ((SH ? (hb >> 16) : hb) & kEntryHash);
                            out_c[count].b = make_uint4(wv[i - 3], wv[i - 2], wv[i - 1], wv[i]);
                        }
                        ++count;
                    }
                }
                anyz = 0xFFFFFFFFu;
                hb = h;
                asm volatile("" : "+v"(hb));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    out_c[0].n = count;
    const uint64_t occ = __builtin_amdgcn_ballot_w64(count != 0);
    if (lane == 0) f.cand_occ[sec] = occ;
}

// ---------------------------------------------------------------- the walk (F2, F3)
// Cursor over the candidate lists of one file, monotone in position. Lists are per unit (sec / 64
// bytes, one F1 lane); unit u of global section s has global index 64 s + u.
struct CandCursor {
    uint64_t sec;   // global unit index of the cursor
    uint32_t idx;   // group index within that unit's list
    uint32_t rsec_idx = 0xFFFFFFFFu;  // the last resolved group (unit + idx) and its flags
    uint64_t rsec = ~0ull;
    uint64_t occ_sec = ~0ull, occ = 0;  // the occupancy mask of section occ_sec (F1's ballot)
    uint32_t rflag = 0, rbits = 0;  // the flag the resolved group's bits are for, and the bits
};

// Full-window hash test of positions [lo, hi) (all inside one file, lo >= 47) by direct byte scan:
// used where a unit's candidate list overflowed. Returns the first position with
// (hash & mask) == 0, or hi.
__device__ uint64_t scan_bytes(const uint8_t* __restrict__ fbase, uint64_t lo, uint64_t hi, uint64_t mask,
                               const uint64_t* __restrict__ gear) {
    // hi <= the file length (queries never pass it)
    uint64_t h = 0;
    for (uint64_t p = lo - kHashSpan; p < hi; p += 16) {
        const uint4 v = load16_file(fbase, p, hi);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint64_t q = p + (uint64_t)j;
            if (q >= hi) return hi;
            h = (h << 1) + gear_of(gear, byte_of(v, j));
            if (q >= lo && (h & mask) == 0) return q;
        }
    }
    return hi;
}

// Exact flags of a candidate group for ONE mask (bit j: position g + j has (hash & mask) == 0): roll
// the 16 bytes F1 stored with it from the hash F1 recorded before it (no re-read of the file: the
// walk is latency-bound and the lists stay in the L2 / Infinity Cache). The tests fold into one
// minimum first; the bits are assembled only when some position hit (always for mask_l, whose bits
// are the ones F1 filtered on; rarely for the stricter mask_s).
__device__ __forceinline__ uint32_t and_or_v(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t resolve_group(const uint4 v, uint64_t g, uint64_t H, uint64_t flen, uint64_t mask,
                                                  const uint64_t* __restrict__ gear) {
    const uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
    uint64_t h = H;
    uint32_t t[16];
    uint32_t z = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        h = (h << 1) + gear_of(gear, byte_of(v, j));
        t[j] = and_or_v((uint32_t)h, mlo, (uint32_t)(h >> 32) & mhi);
        if (j & 1) z = min3_u32(z, t[j - 1], t[j]);
    }
    uint32_t bits = 0;
    if (z == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) bits |= (t[j] == 0 ? 1u : 0u) << j;
    }
    const uint32_t live = flen - g < 16 ? (uint32_t)(flen - g) : 16u;
    return live >= 16 ? bits : bits & ((1u << live) - 1u);
}

// First position in [lo, hi) (file-relative) whose full-window hash matches `flag` (1: mask_s,
// 2: mask_l), or hi. Advances the cursor (callers query increasing positions).
__device__ uint64_t first_cand(const CdcFiles& f, const CdcParams& prm, uint64_t sec0, uint64_t nsec_file,
                               const uint8_t* fbase, uint64_t flen, CandCursor& cur, uint64_t lo, uint64_t hi,
                               uint32_t flag, const uint64_t* gear) {
    if (lo >= hi) return hi;
    // units: the file's sections [sec0, sec0 + nsec_file) hold units [64 sec0, 64 (sec0 + nsec_file))
    const uint64_t u0 = 64 * sec0, nu = 64 * nsec_file;
    const uint64_t s = lo / prm.unit;
    if (cur.sec < u0 + s) {
        cur.sec = u0 + s;
        cur.idx = 0;
    }
    if (cur.sec >= u0 + nu) return hi;
    while (true) {
        // skip the units F1 found no candidate in without loading their counts
        const uint64_t gsec = cur.sec >> 6;
        if (cur.occ_sec != gsec) {
            cur.occ = f.cand_occ[gsec];
            cur.occ_sec = gsec;
        }
        const uint64_t rest = cur.occ >> (cur.sec & 63);
        if (rest == 0) {
            const uint64_t next = (gsec + 1) * 64;  // the next section's first unit
            if (next >= u0 + nu || (next - u0) * prm.unit >= hi) return hi;
            cur.sec = next;
            cur.idx = 0;
            continue;
        }
        if (!(rest & 1)) {
            cur.sec += (uint64_t)__builtin_ctzll(rest);
            cur.idx = 0;
        }
        const uint64_t sec_start = (cur.sec - u0) * prm.unit;  // the unit's start, file-relative
        if (sec_start >= hi) return hi;
        const CandRec* cs = f.cand + cur.sec * prm.cap;
        // an entry and its 16 bytes are loaded together (the bytes before the entry says whether they
        // are needed), and the first pair together with the count (speculatively: slots past the
        // count are scratch, read but never used)
        const uint32_t cnt = (uint32_t)cs[0].n;
        uint64_t e_nx = cur.idx < prm.cap ? cs[cur.idx].e : 0;
        uint4 b_nx = cur.idx < prm.cap ? cs[cur.idx].b : make_uint4(0, 0, 0, 0);
        const uint32_t stored = cnt < prm.cap ? cnt : prm.cap;
        for (bool first = true; cur.idx < stored; first = false) {
            if (!first) {
                e_nx = cs[cur.idx].e;
                b_nx = cs[cur.idx].b;
            }
            const uint64_t e = e_nx;
            const uint4 bv = b_nx;
            const uint64_t g = sec_start + (e >> kEntryShift) * 16;
            if (g >= hi) return hi;
            if (g + 16 > lo) {  // the group overlaps [lo, hi)
                if (cur.rsec != cur.sec || cur.rsec_idx != cur.idx || cur.rflag != flag) {
                    cur.rbits = resolve_group(bv, g, e & kEntryHash, flen, flag == 1 ? prm.mask_s : prm.mask_l, gear);
                    cur.rsec = cur.sec;
                    cur.rsec_idx = cur.idx;
                    cur.rflag = flag;
                }
                uint32_t m = cur.rbits;
                if (lo > g) m &= ~0u << (uint32_t)(lo - g);                  // positions >= lo
                if (hi < g + 16) m &= (1u << (uint32_t)(hi - g)) - 1u;       // positions < hi
                if (m) return g + (uint64_t)__builtin_ctz(m);
                // the rest of the group lies beyond hi: the next query (from hi on) needs it again
                if (g + 16 > hi) return hi;
            }
            // below lo, or done with: later queries start at or after this one's end (an L query
            // follows an S query from eS on), so the group is never needed again
            ++cur.idx;
        }
        const uint64_t sec_end = sec_start + prm.unit;
        if (cnt > prm.cap) {
            // overflowed list: positions after the last stored group were not recorded
            const uint64_t after = stored ? sec_start + (cs[stored - 1].e >> kEntryShift) * 16 + 16 : sec_start;
            const uint64_t a = lo > after ? lo : after;
            const uint64_t b = hi < sec_end ? hi : sec_end;
            if (a < b) {
                const uint64_t m = scan_bytes(fbase, a, b, flag == 1 ? prm.mask_s : prm.mask_l, gear);
                if (m < b) return m;
            }
        }
        // move to the next section only if the query reaches into it: a later query (the L range
        // after an S range) may still need this section
        if (sec_end >= hi || cur.sec + 1 >= u0 + nu) return hi;
        ++cur.sec;
        cur.idx = 0;
    }
}

// Length of the chunk that starts at file-relative position s (cut_gear on content[s..]).
__device__ uint64_t cdc_cut(const CdcFiles& f, const CdcParams& prm, uint64_t sec0, uint64_t nsec_file,
                            const uint8_t* fbase, uint64_t flen, uint64_t s, CandCursor& cur,
                            const uint64_t* gear) {
    if (cut_whole(flen - s, prm)) return flen - s;
    const CutWindow cw = cut_window(flen - s, prm);
    const uint64_t rem = cw.rem, a0 = cw.a0, eS = cw.eS, eL = cw.eL;
    // truncated window: the hash restarts from 0 at a0
    // the 47 bytes from a0: three 16-byte loads issued together
    const uint4 t0 = load16_file(fbase, s + a0, flen), t1 = load16_file(fbase, s + a0 + 16, flen),
                t2 = load16_file(fbase, s + a0 + 32, flen);
    bool exact = true;
    if (a0 + kHashSpan <= eS) {
        // Common case: all 47 positions test mask_s. Roll them with no branch per position (the
        // table reads do not depend on the hash, so they go out ahead) and fold the tests into one
        // minimum; only lanes with a zero test (2^-popcount(mask_s) per position) run the exact loop
        // below to find the first one. The per-position branch with two masks cost ~16 VALU and an
        // LDS round trip per position.
        const uint32_t mlo = (uint32_t)prm.mask_s, mhi = (uint32_t)(prm.mask_s >> 32);
        uint64_t hh = 0;
        uint32_t anyz = 0xFFFFFFFFu, tprev = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < kHashSpan; ++k) {
            const uint32_t b = k < 16 ? byte_of(t0, k) : k < 32 ? byte_of(t1, k - 16) : byte_of(t2, k - 32);
            hh = (hh << 1) + gear_of(gear, b);
            const uint32_t t = and_or((uint32_t)hh, mlo, (uint32_t)(hh >> 32) & mhi);
            if (k & 1) anyz = min3_u32(anyz, tprev, t);
            else tprev = t;
        }
        exact = min_u32(anyz, tprev) == 0;
    }
    if (exact) {
        uint64_t h = 0;
        const uint64_t tend = a0 + kHashSpan < eL ? a0 + kHashSpan : eL;
#pragma unroll
        for (int k = 0; k < kHashSpan; ++k) {
            const uint64_t q = a0 + (uint64_t)k;
            if (q >= tend) break;
            const uint32_t b = k < 16 ? byte_of(t0, k) : k < 32 ? byte_of(t1, k - 16) : byte_of(t2, k - 32);
            h = (h << 1) + gear_of(gear, b);
            if ((h & (q < eS ? prm.mask_s : prm.mask_l)) == 0) return q;
        }
    }
    // [qs, eS) against mask_s, then [max(qs, eS), eL) against mask_l, through ONE first_cand site: the
    // lanes of a wave in either range run it together, and the walk's code (and its register
    // pressure) is half the size of two inlined copies
    const uint64_t qs = a0 + kHashSpan;
#pragma unroll 1
    for (uint32_t flag = 1; flag <= 2; ++flag) {
        const uint64_t lo = flag == 1 ? qs : (qs > eS ? qs : eS);
        const uint64_t hi = flag == 1 ? eS : eL;
        if (lo < hi) {
            const uint64_t p = first_cand(f, prm, sec0, nsec_file, fbase, flen, cur, s + lo, s + hi, flag, gear);
            if (p < s + hi) return p - s;
        }
    }
    return rem;
}

// F2: speculative walk of one section from its start, recording chunk starts (relative to the
// section start) until a start reaches the section end or the file end (that start is recorded too).
__global__ __launch_bounds__(256) void cdc_walk_kernel(CdcFiles f, CdcParams prm, uint64_t n_sec) {
    __shared__ uint64_t lds_gear[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lds_gear[i] = kGear[i];
    __syncthreads();
    const uint64_t sec = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sec >= n_sec) return;
    const uint32_t file = f.sec_file[sec];
    const uint64_t flen = f.flen[file];
    const uint64_t sec0 = f.sec_base[file], nsec_file = f.sec_base[file + 1] - sec0;
    const uint64_t sec_start = (sec - sec0) * prm.sec;
    const uint64_t sec_end = sec_start + prm.sec < flen ? sec_start + prm.sec : flen;
    const uint8_t* fbase = f.arena + f.foff[file];
    uint32_t* out = f.spec + sec * prm.speccap;
    // warm up over the `warmup` bytes before the section (unrecorded): a walk started anywhere meets
    // the true walk within a few chunks, so the recorded starts are almost always the true ones
    // One loop for the warm-up and the recorded part (one cdc_cut site): each lane moves from one to
    // the other on its own, instead of the wave finishing every lane's warm-up first.
    uint64_t s = sec_start > prm.warmup ? sec_start - prm.warmup : 0;
    CandCursor cur{64 * sec0 + s / prm.unit, 0};
    uint32_t n = 0;
    while (true) {
        if (s >= sec_start) {
            if (n < prm.speccap) out[n] = (uint32_t)(s - sec_start);
            ++n;
            if ((s >= sec_end && n > 1) || s >= flen) break;
        }
        s += cdc_cut(f, prm, sec0, nsec_file, fbase, flen, s, cur, lds_gear);
    }
    f.spec_cnt[sec] = n;
}

// ---------------------------------------------------------------- F3: stitch
// Sections are at least `max` bytes, so every chunk that starts before a section ends at or before
// the next section's end: the true walk's first start in section i, entry(i), is < sec_end(i).
// If section i-1 is right, entry(i) is the last start its list recorded (the first >= its end). When
// that start also appears in section i's speculative list, everything after it in that list is the
// true walk (a cut depends only on where its chunk starts) -- section i "converged". Induction from
// section 0 (which starts at the file start, so its walk is the true one) makes every converged
// section right, except after a section that did not converge; those are re-walked serially (F3b).
__device__ __forceinline__ uint64_t spec_last_abs(const CdcFiles& f, const CdcParams& prm, uint64_t sec,
                                                  uint64_t sec_start) {
    return sec_start + f.spec[sec * prm.speccap + (f.spec_cnt[sec] - 1)];
}

// F3a: one lane per section.
__global__ __launch_bounds__(256) void cdc_check_kernel(CdcFiles f, CdcParams prm, CdcStitch s, uint64_t n_sec) {
    const uint64_t sec = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sec >= n_sec) return;
    const uint32_t file = f.sec_file[sec];
    const uint64_t sec0 = f.sec_base[file];
    const uint64_t sec_start = (sec - sec0) * prm.sec;
    const uint32_t cnt = f.spec_cnt[sec];
    const uint32_t* spec = f.spec + sec * prm.speccap;
    uint32_t status = kFailed, k0 = 0;
    if (cnt <= prm.speccap) {
        if (sec == sec0) {
            status = kConverged;
        } else if (f.spec_cnt[sec - 1] <= prm.speccap) {
            const uint64_t e = spec_last_abs(f, prm, sec - 1, sec_start - prm.sec);
            // binary search e - sec_start in the sorted list
            uint32_t lo = 0, hi = cnt;
            const uint64_t key = e - sec_start;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((uint64_t)spec[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            if (lo < cnt && (uint64_t)spec[lo] == key) {
                status = kConverged;
                k0 = lo;
            }
        }
    }
    s.status[sec] = status;
    s.k0[sec] = k0;
    if (status == kConverged) {
        s.count[sec] = cnt - 1 - k0;  // every entry but the last is a start inside the section
        s.exit[sec] = sec_start + spec[cnt - 1];
    }
}

// F3b: one wave per file finds the sections that did not converge (64 statuses per step) and its
// lane 0 re-walks them: from the true entry, cut chunks until a start lands on the section's
// speculative list (the rest of the list is then right) or the walk leaves the section (then the
// next section's check is void and it is re-walked too).
__global__ __launch_bounds__(64) void cdc_fixup_kernel(CdcFiles f, CdcParams prm, CdcStitch s, uint64_t n_files) {
    __shared__ uint64_t lds_gear[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lds_gear[i] = kGear[i];
    __syncthreads();
    const uint64_t file = blockIdx.x;
    if (file >= n_files) return;
    const int lane = threadIdx.x;
    const uint64_t flen = f.flen[file];
    const uint64_t sec0 = f.sec_base[file], nsec_file = f.sec_base[file + 1] - sec0;
    const uint8_t* fbase = f.arena + f.foff[file];
    uint64_t i = 1;  // section 0 always converges
    while (i < nsec_file) {
        // next failed section at or after i
        const uint64_t j = i + (uint64_t)lane;
        const bool failed = j < nsec_file && s.status[sec0 + j] == kFailed;
        const uint64_t m = __builtin_amdgcn_ballot_w64(failed);
        if (m == 0) {
            i += 64;
            continue;
        }
        i += (uint64_t)__builtin_ctzll(m);
        // lane 0 re-walks from section i; the others wait at the next ballot
        uint64_t next = i;
        if (lane == 0) {
            uint64_t pos = s.exit[sec0 + i - 1];
            CandCursor cur{64 * (sec0 + i), 0};
            for (uint64_t t = i; t < nsec_file; ++t) {
                const uint64_t sec = sec0 + t;
                const uint64_t sec_start = t * prm.sec;
                const uint64_t sec_end = sec_start + prm.sec < flen ? sec_start + prm.sec : flen;
                const uint32_t cnt = f.spec_cnt[sec];
                const uint32_t* spec = f.spec + sec * prm.speccap;
                const bool spec_ok = cnt <= prm.speccap;
                uint32_t* fix = s.fix + sec * prm.speccap;
                uint32_t n = 0, k = 0;
                bool landed = false;
                while (pos < sec_end) {
                    if (spec_ok) {
                        while (k < cnt && sec_start + spec[k] < pos) ++k;
                        if (k < cnt && sec_start + spec[k] == pos) {
                            for (; k + 1 < cnt; ++k) fix[n++] = spec[k];
                            pos = sec_start + spec[cnt - 1];
                            landed = true;
                            break;
                        }
                    }
                    fix[n++] = (uint32_t)(pos - sec_start);
                    if (cur.sec < 64 * sec) cur = CandCursor{64 * sec, 0};
                    pos += cdc_cut(f, prm, sec0, nsec_file, fbase, flen, pos, cur, lds_gear);
                }
                s.status[sec] = kFixed;
                s.count[sec] = n;
                s.exit[sec] = pos;
                next = t + 1;
                // a converged next section is right only if its check saw this exit
                if (landed && (t + 1 >= nsec_file || s.status[sec + 1] == kConverged)) break;
            }
        }
        i = (uint64_t)__builtin_amdgcn_readfirstlane((int)next) | ((uint64_t)__builtin_amdgcn_readfirstlane((int)(next >> 32)) << 32);
    }
}

// F1: one wave per section (kScanWaves per workgroup, 160 KiB of LDS); SH when the bits both masks
// share are all >= 16. Then F2, F3a and F3b.
hipError_t cdc_launch_scan(const CdcFiles& f, const CdcParams& prm, const CdcStitch& s, uint64_t n_sec, uint64_t n_files,
                           hipStream_t st) {
    const bool sh = (((prm.mask_s & prm.mask_l) << 16) & 0xFFFFFFFFull) == 0;
    auto scan = sh ? cdc_scan_kernel<true> : cdc_scan_kernel<false>;
    constexpr int wv = kScanWaves;
    hipLaunchKernelGGL(scan, dim3((unsigned)((n_sec + wv - 1) / wv)), dim3(64 * wv), 0, st, f, prm, n_sec);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cdc_walk_kernel, dim3((unsigned)((n_sec + 255) / 256)), dim3(256), 0, st, f, prm, n_sec);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cdc_check_kernel, dim3((unsigned)((n_sec + 255) / 256)), dim3(256), 0, st, f, prm, s, n_sec);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cdc_fixup_kernel, dim3((unsigned)n_files), dim3(64), 0, st, f, prm, s, n_files);
    return hipGetLastError();
}

}  // namespace oxh
