// oxen_amd/csrc/snappy_compress.hip -- many blocks compressed to raw Snappy streams per launch (oxh_snappy_compress_*).
// The format, the bound and the entries' contract are stated in include/oxen_hash.h "Snappy, compress"; the entries'
// checks are capi_dispatch.hip's.
//
// A block is cut into fragments of at most 64 KiB and a copy never reaches outside its fragment, so fragments
// compress independently and a 2-byte offset always suffices (the reference Snappy makes the same cut). The unit of
// parallelism is the fragment: one wave per fragment, workgroups of one wave, a capped grid that loops over the
// fragments -- the shape of snappy_inflate_kernel. Fragment f compresses into slot f of a scratch the call owns
// (snc::kSlot bytes each: below); a second kernel, a wave per block, writes the block's preamble and copies its
// fragments' streams one behind the other into the caller's destination.
//
// Per fragment the wave walks the input in batches of 64 consecutive positions, a position a lane:
//   probe    the lane hashes the 4 bytes at its position (multiplicative), reads its candidate from a table of
//            2^12 positions in LDS and then enters its own position with an LDS atomic max: every read of a batch
//            comes before every insert of it, and a slot's content after the batch is the largest position entered,
//            whichever lane's operation ran last. The entries are 32 bits wide because LDS atomics are (the positions
//            need 16): 16 KiB a wave. A cleared slot reads as position 0, which is a candidate like any other: a
//            candidate counts only when it lies in front of the lane's position and its 4 bytes, loaded from the
//            input, are equal;
//   extend   every lane with a candidate extends its own match 8 bytes at a time up to snc::kLaneCap bytes or the
//            fragment's end;
//   select   a loop over the set bits of the ballot of matches, uniform in the wave, keeps a cursor -- the first input
//            byte not yet covered -- takes the first match at or behind it, moves the cursor to the match's end and
//            drops the bits in front of it: greedy, not overlapping, one step per match taken. A taken match that
//            reached the cap is extended there by the whole wave, 64 lanes x 8 bytes per round and a ballot of the
//            lanes that saw a mismatch or the end (constant pages are one such match);
//   emit     a taken lane owns the literal in front of its match and its copy elements (2 bytes where length <= 11 and
//            offset < 2 048, else 3 bytes per 64). Of a batch only the first literal (the bytes pending since the last
//            match) and the last copy can be long -- every other taken match ends inside the batch. A first literal
//            above snc::kLitStage bytes is copied by the whole wave straight from the input (an incompressible
//            fragment is one such literal); a last copy above 64 bytes is written by the wave, an element a lane;
//            everything else is placed by a wave prefix sum of its sizes, assembled in an LDS staging buffer at the
//            destination's own misalignment and stored 16 bytes a lane on the destination's 16-byte grid;
//   advance  the next batch starts at the cursor; a batch without a match moves on and the pending literal grows: by
//            64, and after every 16 barren batches in a row by twice as much, up to 512 (the positions skipped are
//            neither probed nor entered); a match sets the stride back.
// Matches whose candidate lies inside the lane's own batch are not found (the reads come before the inserts).
//
// The slot. A literal of g bytes costs g + 1, + 2 above 60 and + 3 above 256; a copy of m >= 4 bytes costs at most
// 3 per 64, never more than m - 1. So a literal and the copy behind it grow the stream by at most 2 bytes and only
// when the literal has more than 60: a fragment of n bytes gives at most n + n / 65 + 3 <= 66 548 bytes. Every store
// is still checked against the slot first; a fragment that would pass it ends the call with an error.
// Nothing is read outside the block's own [src_lo, src_hi) and nothing is written outside its [dst_lo, dst_hi). The
// same input gives the same bytes: nothing depends on the order of lanes, waves or stores.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "snappy_wave.hpp"

namespace oxh {

// The two parameters tools/snappy_compress_probe.py chose (DESIGN.md §4 "Snappy, compress" has the arms); the probe
// builds the other arms of its comparison by defining them.
#ifndef OXH_SNAPPY_TABLE_BITS
#define OXH_SNAPPY_TABLE_BITS 12
#endif
#ifndef OXH_SNAPPY_WIDEN
#define OXH_SNAPPY_WIDEN 1
#endif

namespace snc {
constexpr uint32_t kFragment = kSnappyFragment;
constexpr uint32_t kSlot = kSnappySlot;
constexpr uint32_t kTableBits = OXH_SNAPPY_TABLE_BITS;  // 16 KiB of LDS a wave; the grid cap, not LDS, bounds residency at 8 waves a CU
constexpr bool kWiden = OXH_SNAPPY_WIDEN;  // the stride over barren input doubles every 16 barren batches, up to 8 x 64
constexpr uint32_t kLaneCap = 64;        // a lane extends its own match to 4 + a multiple of 8 at or above this
constexpr uint32_t kLitStage = 64;       // a batch's first literal above this is the whole wave's
constexpr uint32_t kStage = 1024;        // the staging buffer: a batch's short elements (below 448 bytes), 256 copy elements
constexpr unsigned kMaxGroups = 2048;
constexpr uint32_t kOverflow = 0xFFFFFFFFu;  // frag_size of a fragment that would have passed its slot
static_assert(kFragment + kFragment / 65 + 3 <= kSlot && kSlot % 16 == 0, "the slot holds a fragment's worst case");
}  // namespace snc

__device__ __forceinline__ uint32_t snc_lit_head(uint32_t g) { return g <= 60 ? 1 : g <= 256 ? 2 : 3; }

// The tag of a literal of 1 <= g <= 65 536 bytes, by one lane.
__device__ __forceinline__ void snc_put_lit_head(uint8_t* p, uint32_t g) {
    if (g <= 60) {
        p[0] = (uint8_t)((g - 1) << 2);
    } else if (g <= 256) {
        p[0] = 60 << 2, p[1] = (uint8_t)(g - 1);
    } else {
        p[0] = 61 << 2, p[1] = (uint8_t)(g - 1), p[2] = (uint8_t)((g - 1) >> 8);
    }
}

// A copy of 1 <= len <= 64 bytes with a 2-byte offset.
__device__ __forceinline__ void snc_put_copy2(uint8_t* p, uint32_t len, uint32_t back) {
    p[0] = (uint8_t)(2 | (len - 1) << 2), p[1] = (uint8_t)back, p[2] = (uint8_t)(back >> 8);
}

// The n <= snc::kStage bytes staged from stage[d & 15] on to d[0 .. n): 16 bytes a lane on d's 16-byte grid, the
// blocks that hold the span's head or tail byte by byte.
__device__ __forceinline__ void snc_store_span(uint8_t* d, uint32_t n, const uint8_t* stage, unsigned lane) {
    const uintptr_t d0 = (uintptr_t)d, d1 = d0 + n, grid0 = d0 & ~(uintptr_t)15;
    for (uint32_t b = 16 * lane; grid0 + b < d1; b += 16 * 64) {
        const uintptr_t to = grid0 + b;
        if (to >= d0 && to + 16 <= d1) {
            *reinterpret_cast<uint4*>(to) = *reinterpret_cast<const uint4*>(&stage[b]);
        } else {
            for (uint32_t k = 0; k < 16; ++k)
                if (to + k >= d0 && to + k < d1) *reinterpret_cast<uint8_t*>(to + k) = stage[b + k];
        }
    }
}

// The match of in[at ..) with in[cand ..), equal over `len` bytes so far, extended by the whole wave to its end or
// the fragment's: its full length.
__device__ __forceinline__ uint32_t snc_extend_wave(const uint8_t* in, uint32_t n, uint32_t cand, uint32_t at, uint32_t len, unsigned lane) {
    const uint32_t back = at - cand;
    for (;;) {  // uniform in the wave
        const uint32_t p = at + len + 8 * lane;
        uint32_t eq = 0;  // the equal bytes of the lane's 8
        if (p + 8 <= n) {
            const uint64_t x = ld64u(in + p) ^ ld64u(in + p - back);
            eq = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8;
        } else {
            while (p + eq < n && in[p + eq] == in[p + eq - back]) ++eq;
        }
        const unsigned long long stop = __ballot(eq < 8);
        if (stop) {
            const int j = __builtin_ctzll(stop);
            return len + 8 * j + __shfl(eq, j, 64);
        }
        len += 512;
    }
}

// Fragment f = block frag_block[f]'s bytes [k * 64 KiB, (k + 1) * 64 KiB), k = f - frag0[block], compressed into
// slots[f * kSlot ..); frag_size[f] = the stream's bytes, or snc::kOverflow (ctrl[0] |= 1).
__global__ __launch_bounds__(64) void snappy_compress_kernel(const uint8_t* __restrict__ src_all, const uint64_t* __restrict__ src_lo,
                                                             const uint64_t* __restrict__ src_hi, const uint32_t* __restrict__ frag_block,
                                                             const uint64_t* __restrict__ frag0, uint64_t nfrags, uint8_t* __restrict__ slots,
                                                             uint32_t* __restrict__ frag_size, unsigned long long* __restrict__ ctrl) {
    __shared__ __attribute__((aligned(16))) uint32_t table[1u << snc::kTableBits];
    __shared__ __attribute__((aligned(16))) uint8_t stage[snc::kStage + 16];
    const unsigned lane = threadIdx.x;
    bool any_over = false;
    for (uint64_t f = blockIdx.x; f < nfrags; f += gridDim.x) {  // uniform in the wave
        const uint32_t b = frag_block[f];
        const uint64_t s0 = src_lo[b], s1 = src_hi[b], at = (f - frag0[b]) * snc::kFragment;
        if (s1 < s0 || at >= s1 - s0) {  // not a fragment of the block as it stands now: nothing is read
            if (lane == 0) frag_size[f] = 0;
            continue;
        }
        const uint32_t n = (uint32_t)(s1 - s0 - at < snc::kFragment ? s1 - s0 - at : snc::kFragment);
        const uint8_t* const in = src_all + s0 + at;
        uint8_t* const out = slots + f * snc::kSlot;
        snp_lds_order();  // the fragment before is done with the table
        for (uint32_t i = 4 * lane; i < (1u << snc::kTableBits); i += 256) *reinterpret_cast<uint4*>(&table[i]) = uint4{0, 0, 0, 0};
        snp_lds_order();
        uint32_t p0 = 0;    // the batch's first position
        uint32_t lit0 = 0;  // the first byte not yet emitted: the pending literal is [lit0, p0)
        uint32_t op = 0;    // the slot's bytes so far
        uint32_t barren = 0;  // the batches without a match since the last one
        bool over = false;
        while (p0 + 4 <= n) {  // uniform in the wave
            const uint32_t my = p0 + lane;
            const bool have = my + 4 <= n;
            const uint32_t w = have ? ld32u(in + my) : 0;
            const uint32_t h = (w * 0x1E35A7BDu) >> (32 - snc::kTableBits);
            uint32_t cand = have ? table[h] : 0;
            snp_lds_order();  // every read of the batch, then its inserts
            if (have) atomicMax(&table[h], my);
            snp_lds_order();
            const bool has = have && cand < my && ld32u(in + cand) == w;
            const uint32_t back = my - cand;
            uint32_t len = 0;
            bool open = false;  // no mismatch and no end seen yet: the match reached the cap
            if (has) {
                len = 4, open = true;
                while (open && len < snc::kLaneCap) {
                    if (my + len + 8 <= n) {
                        const uint64_t x = ld64u(in + my + len) ^ ld64u(in + my + len - back);
                        if (x)
                            len += (uint32_t)__builtin_ctzll(x) >> 3, open = false;
                        else
                            len += 8;
                    } else {
                        while (my + len < n && in[my + len] == in[my + len - back]) ++len;
                        open = false;
                    }
                }
            }
            unsigned long long bits = __ballot(has);
            if (!bits) {  // a barren batch: the pending literal grows
                p0 += snc::kWiden ? 64u << (barren >> 4 < 3 ? barren >> 4 : 3) : 64u;
                ++barren;
                continue;
            }
            // select: greedy and not overlapping, a step per match taken
            uint32_t cur = p0, gap_from = lit0, gap = 0;
            bool sel = false;
            while (bits) {  // uniform in the wave
                const int i = __builtin_ctzll(bits);
                uint32_t li = __shfl(len, i, 64);
                if (__shfl((int)open, i, 64)) li = snc_extend_wave(in, n, __shfl(cand, i, 64), p0 + i, li, lane);
                li = __builtin_amdgcn_readfirstlane(li);  // the same in every lane: the cursor stays scalar
                if ((int)lane == i) sel = true, len = li, gap = gap_from;
                cur = p0 + i + li, gap_from = cur;
                bits = cur - p0 >= 64 ? 0 : bits & (~0ull << (cur - p0));
            }
            const unsigned long long chosen = __ballot(sel);
            const int first = __builtin_ctzll(chosen), last = 63 - __builtin_clzll(chosen);
            const uint32_t g = sel ? my - gap : 0;  // the literal in front of the lane's match
            // the first literal, where it is long: the whole wave, straight from the input
            const uint32_t g0 = __shfl(g, first, 64);
            if (g0 > snc::kLitStage) {
                const uint32_t hd = snc_lit_head(g0);
                if (op + hd + g0 > snc::kSlot) {
                    over = true;
                    break;
                }
                if (lane == 0) snc_put_lit_head(out + op, g0);
                snp_span_wave<false>(out + op + hd, in + lit0, g0, lane);
                op += hd + g0;
            }
            // the short elements: a prefix sum of their sizes places them in the staging buffer
            const bool lit = sel && g && !((int)lane == first && g0 > snc::kLitStage);
            const bool big = sel && len > 64;  // only the last taken match can be
            const bool near = len <= 11 && back < 2048;
            const uint32_t size = (lit ? snc_lit_head(g) + g : 0) + (sel && !big ? (near ? 2u : 3u) : 0);
            uint32_t incl = size;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t below = __shfl_up(incl, off, 64);
                if ((int)lane >= off) incl += below;
            }
            const uint32_t total = __shfl(incl, 63, 64);
            if (total) {
                if (total > snc::kStage || op + total > snc::kSlot) {
                    over = true;
                    break;
                }
                uint8_t* p = stage + ((uintptr_t)(out + op) & 15) + incl - size;
                if (lit) {
                    const uint32_t hd = snc_lit_head(g);
                    snc_put_lit_head(p, g);
                    copy_span_lane(p + hd, in + gap, g);
                    p += hd + g;
                }
                if (sel && !big) {
                    if (near)
                        p[0] = (uint8_t)(1 | (len - 4) << 2 | (back >> 8) << 5), p[1] = (uint8_t)back;
                    else
                        snc_put_copy2(p, len, back);
                }
                snp_lds_order();  // the batch is assembled
                snc_store_span(out + op, total, stage, lane);
                snp_lds_order();  // and stored: the buffer may be overwritten
                op += total;
            }
            // the last copy, where it is long: 64 bytes an element, an element a lane
            if (__ballot(big)) {
                const uint32_t L = __shfl(len, last, 64), o = __shfl(back, last, 64), count = (L + 63) / 64;
                if (op + 3 * count > snc::kSlot) {
                    over = true;
                    break;
                }
                for (uint32_t e0 = 0; e0 < count; e0 += 256) {
                    const uint32_t cnt = count - e0 < 256 ? count - e0 : 256;
                    uint8_t* const p = stage + ((uintptr_t)(out + op) & 15);
                    for (uint32_t k = lane; k < cnt; k += 64) snc_put_copy2(p + 3 * k, e0 + k + 1 < count ? 64 : L - 64 * (count - 1), o);
                    snp_lds_order();
                    snc_store_span(out + op, 3 * cnt, stage, lane);
                    snp_lds_order();
                    op += 3 * cnt;
                }
            }
            lit0 = cur, p0 = cur, barren = 0;
        }
        if (!over && lit0 < n) {  // what is left is a literal
            const uint32_t g = n - lit0, hd = snc_lit_head(g);
            if (op + hd + g > snc::kSlot) {
                over = true;
            } else {
                if (lane == 0) snc_put_lit_head(out + op, g);
                snp_span_wave<false>(out + op + hd, in + lit0, g, lane);
                op += hd + g;
            }
        }
        if (lane == 0) frag_size[f] = over ? snc::kOverflow : op;
        any_over |= over;
    }
    if (lane == 0 && any_over) __hip_atomic_fetch_or(&ctrl[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Block b's stream to dst_all[dst_lo[b] ..): the preamble, then the streams of its fragments frag0[b] .. frag0[b + 1)
// out of their slots. sizes[b] = the stream's bytes and status[b] = 0; or OXH_SNAPPY_RANGE and sizes[b] = 0, with
// nothing written: offsets that decrease, a block of 2^32 bytes or more, a destination below the stream -- `strict`:
// below snappy_bound() of the block --, fragments that are not the block's (ctrl[0] |= 2) or that passed their slot.
__global__ __launch_bounds__(64) void snappy_pack_kernel(const uint64_t* __restrict__ src_lo, const uint64_t* __restrict__ src_hi, uint8_t* dst_all,
                                                         const uint64_t* __restrict__ dst_lo, const uint64_t* __restrict__ dst_hi,
                                                         const uint64_t* __restrict__ frag0, const uint8_t* __restrict__ slots,
                                                         const uint32_t* __restrict__ frag_size, uint64_t* __restrict__ sizes,
                                                         uint32_t* __restrict__ status, uint64_t nblocks, int strict,
                                                         unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {  // uniform in the wave
        const uint64_t s0 = src_lo[b], s1 = src_hi[b], d0 = dst_lo[b], d1 = dst_hi[b], f0 = frag0[b], f1 = frag0[b + 1];
        const uint64_t n = s1 - s0, room = d1 - d0;
        bool ok = s1 >= s0 && d1 >= d0 && n <= 0xFFFFFFFFull && !(strict && room < snappy_bound(n));
        uint64_t need = 0;
        if (ok && (f1 < f0 || f1 - f0 != snappy_fragments(n))) {
            ok = false;
            if (lane == 0) __hip_atomic_fetch_or(&ctrl[0], 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        uint32_t plen = 1;
        if (ok) {
            bool over = false;
            for (uint64_t f = f0 + lane; f < f1; f += 64) {
                const uint32_t size = frag_size[f];
                over |= size > snc::kSlot;
                need += size;
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) need += (uint64_t)__shfl_xor((long long)need, off, 64);
            while (n >> (7 * plen)) ++plen;
            need += plen;
            ok = !__ballot(over) && need <= room;
        }
        if (!ok) {
            if (lane == 0) status[b] = OXH_SNAPPY_RANGE, sizes[b] = 0;
            continue;
        }
        uint8_t* const dst = dst_all + d0;
        if (lane < plen) dst[lane] = (uint8_t)(((n >> (7 * lane)) & 127) | (lane + 1 < plen ? 128 : 0));
        uint64_t pos = plen;
        for (uint64_t f = f0; f < f1; ++f) {
            const uint32_t size = frag_size[f];
            snp_span_wave<false>(dst + pos, slots + f * snc::kSlot, size, lane);
            pos += size;
        }
        if (lane == 0) status[b] = 0, sizes[b] = pos;
    }
}

__global__ void snappy_compress_clear_kernel(unsigned long long* word) { *word = 0; }

int snappy_fragments_enqueue(const uint8_t* d_src, const uint64_t* d_src_lo, const uint64_t* d_src_hi, const SnappyWork& w, hipStream_t st) {
    using namespace oxh::capi;
    snappy_compress_clear_kernel<<<1, 1, 0, st>>>(w.d_ctrl);
    HIP_TRY(hipGetLastError());
    if (!w.nfrags) return OXH_OK;
    const unsigned grid = (unsigned)std::min<uint64_t>(w.nfrags, snc::kMaxGroups);
    snappy_compress_kernel<<<grid, 64, 0, st>>>(d_src, d_src_lo, d_src_hi, w.d_frag_block, w.d_frag0, w.nfrags, w.d_slots, w.d_frag_size, w.d_ctrl);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

int snappy_pack_enqueue(const uint64_t* d_src_lo, const uint64_t* d_src_hi, uint8_t* d_dst, const uint64_t* d_dst_lo, const uint64_t* d_dst_hi,
                        uint64_t* d_sizes, uint32_t* d_status, uint64_t nblocks, bool strict, const SnappyWork& w, hipStream_t st) {
    using namespace oxh::capi;
    const unsigned grid = (unsigned)std::min<uint64_t>(nblocks, snc::kMaxGroups);
    snappy_pack_kernel<<<grid, 64, 0, st>>>(d_src_lo, d_src_hi, d_dst, d_dst_lo, d_dst_hi, w.d_frag0, w.d_slots, w.d_frag_size, d_sizes, d_status,
                                            nblocks, strict ? 1 : 0, w.d_ctrl);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

}  // namespace oxh
