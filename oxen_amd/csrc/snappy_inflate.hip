// oxen_amd/csrc/snappy_inflate.hip -- many raw Snappy blocks inflated per launch (oxh_snappy_inflate_*, and the
// Parquet open's SNAPPY pages: parquet_read.hip). The format and the cause codes are stated in include/oxen_hash.h
// "Snappy"; the entries' checks are capi_dispatch.hip's.
//
// One wave per block, workgroups of one wave, a capped grid that loops over the blocks -- the shape of
// pq_chase_kernel (parquet_read.hip), whose serial length chain is the same problem: the tags are found only one
// from the other, the bytes they name are not. Per block:
//   window   the wave loads the block's input through LDS in 1 KiB windows, 16 bytes a lane, at any alignment; every
//            load stays inside the block's own [src, src + n);
//   chase    one lane walks the tags whose whole header (the tag and at most 4 more bytes) lies inside the window into
//            up to 64 cells (kind, source, length, destination) in LDS. A literal's payload may run past the window:
//            its cell names the payload in the input. The lane stops at 64 cells or at a header that leaves the
//            window; the next window starts at the first tag it did not parse, so no header straddles two windows;
//   execute  the whole wave, a cell a lane. Literals depend on nothing written: all of the batch go first, a lane
//            per cell below 256 bytes, the whole wave in aligned 16-byte stores from there (an incompressible page is
//            one such literal). Copies run in rounds: a copy is ready when its source range ends at or before the
//            destination of the first copy still pending -- everything in front of that is written. A copy that
//            overlaps itself reads out[dst - offset + i % offset], which is all in front of its own destination, so
//            the first pending copy is always ready and every round retires a cell. A ballot picks the ready cells;
//            between rounds a workgroup-scope release / acquire fence makes the wave's stores visible to its loads.
//            History is read from global memory (hot in L2).
// A malformed stream sets the block's status to its cause and ends the block; the block's whole destination is then
// zeros. No byte outside [dst, dst + want) is written: an element is checked against what is left of the declared
// length before its cell exists. A copy's source is inside [0, produced) before any load: 0 < offset <= produced.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "snappy_wave.hpp"  // snp_lds_order, snp_global_order, snp_span_wave

namespace oxh {

namespace snp {
constexpr uint32_t kWindow = 1024;       // bytes of input the chase looks at at once: 64 lanes x 16
constexpr uint32_t kBatch = 64;          // cells of one chase: a lane each
constexpr uint32_t kLongLiteral = 256;   // a literal of this many bytes and more is the whole wave's
constexpr unsigned kSnappyMaxGroups = 2048;
constexpr uint32_t kLiteral = 0, kCopy = 1, kNone = 2;
}  // namespace snp

// Block b: src_all[src_lo[b], src_hi[b]) inflates to dst_all[dst_lo[b], dst_hi[b]); status[b] = 0 or the cause;
// bad_count += the blocks with a cause.
__global__ __launch_bounds__(64) void snappy_inflate_kernel(const uint8_t* __restrict__ src_all, const uint64_t* __restrict__ src_lo,
                                                            const uint64_t* __restrict__ src_hi, uint8_t* dst_all,
                                                            const uint64_t* __restrict__ dst_lo, const uint64_t* __restrict__ dst_hi,
                                                            uint32_t* __restrict__ status, uint64_t nblocks,
                                                            unsigned long long* __restrict__ bad_count) {
    __shared__ uint8_t win[snp::kWindow];
    __shared__ uint64_t cell_src[snp::kBatch];  // a literal: where its payload starts in the input; a copy: its offset
    __shared__ uint32_t cell_len[snp::kBatch], cell_dst[snp::kBatch], cell_kind[snp::kBatch];
    const unsigned lane = threadIdx.x;
    unsigned long long bad = 0;
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {  // uniform in the wave
        const uint64_t s0 = src_lo[b], s1 = src_hi[b], d0 = dst_lo[b], d1 = dst_hi[b];
        if (s1 < s0 || d1 < d0) {  // no range to read or to fill
            if (lane == 0) status[b] = OXH_SNAPPY_RANGE;
            ++bad;
            continue;
        }
        const uint8_t* src = src_all + s0;
        uint8_t* dst = dst_all + d0;
        const uint64_t n = s1 - s0, want = d1 - d0;
        uint32_t err = 0;
        // the preamble: the same bytes in every lane
        uint64_t cur = 0, declared = 0;
        bool ended = false;
        for (uint32_t i = 0; i < 5 && cur < n && !ended; ++i) {
            const uint32_t byte = src[cur++];
            declared |= (uint64_t)(byte & 127) << (7 * i);
            ended = !(byte & 128);
        }
        if (!ended || declared > 0xFFFFFFFFull || declared != want) err = OXH_SNAPPY_PREAMBLE;
        uint64_t produced = 0;  // below 2^32 from here on: want is
        while (!err && cur < n) {
            const uint32_t wlen = (uint32_t)(n - cur < snp::kWindow ? n - cur : snp::kWindow);
            snp_lds_order();  // the window and the cells before have been read
            if (16 * lane + 16 <= wlen) {
                const uint64_t lo = ld64u(src + cur + 16 * lane), hi = ld64u(src + cur + 16 * lane + 8);
                __builtin_memcpy(win + 16 * lane, &lo, 8);
                __builtin_memcpy(win + 16 * lane + 8, &hi, 8);
            } else {
                for (uint32_t k = 16 * lane; k < wlen && k < 16 * lane + 16; ++k) win[k] = src[cur + k];
            }
            snp_lds_order();
            uint32_t k = 0, cause = 0;
            uint64_t pos = 0, made = produced;
            if (lane == 0) {
                while (k < snp::kBatch && pos < wlen) {
                    const uint32_t tag = win[pos], form = tag & 3;
                    const uint32_t extra = form == 0 ? ((tag >> 2) >= 60 ? (tag >> 2) - 59 : 0) : form == 1 ? 1 : form == 2 ? 2 : 4;
                    if (pos + 1 + extra > wlen) {
                        if (cur + pos + 1 + extra > n) cause = OXH_SNAPPY_INPUT;  // the header leaves the input
                        break;                                                    // else: the next window starts at this tag
                    }
                    uint32_t x = 0;
                    for (uint32_t i = 0; i < extra; ++i) x |= (uint32_t)win[pos + 1 + i] << (8 * i);
                    uint64_t len;
                    if (form == 0) {
                        len = (uint64_t)(extra ? x : tag >> 2) + 1;
                        const uint64_t at = cur + pos + 1 + extra;
                        if (len > n - at) cause = OXH_SNAPPY_INPUT;
                        else if (len > want - made) cause = OXH_SNAPPY_OVERRUN;
                        if (cause) break;
                        cell_kind[k] = snp::kLiteral, cell_src[k] = at;
                        pos += 1 + extra + len;
                    } else {
                        uint32_t off = x;
                        len = (tag >> 2) + 1;
                        if (form == 1) len = 4 + ((tag >> 2) & 7), off = ((tag >> 5) << 8) | x;
                        if (off == 0) cause = OXH_SNAPPY_OFFSET_ZERO;
                        else if (off > made) cause = OXH_SNAPPY_OFFSET_BEYOND;
                        else if (len > want - made) cause = OXH_SNAPPY_OVERRUN;
                        if (cause) break;
                        cell_kind[k] = snp::kCopy, cell_src[k] = off;
                        pos += 1 + extra;
                    }
                    cell_len[k] = (uint32_t)len, cell_dst[k] = (uint32_t)made;
                    made += len, ++k;
                }
            }
            snp_lds_order();
            k = __shfl(k, 0, 64), cause = __shfl(cause, 0, 64);
            pos = (uint64_t)__shfl((long long)pos, 0, 64), made = (uint64_t)__shfl((long long)made, 0, 64);
            if (cause) {  // (a batch without a cell has a cause: a window starts at a tag and holds its header or ends the input)
                err = cause;
                break;
            }
            const uint32_t kind = lane < k ? cell_kind[lane] : snp::kNone;
            const uint64_t from = lane < k ? cell_src[lane] : 0;
            const uint32_t len = lane < k ? cell_len[lane] : 0, at = lane < k ? cell_dst[lane] : 0;
            // literals: nothing they read is written here
            const bool is_long = kind == snp::kLiteral && len >= snp::kLongLiteral;
            if (kind == snp::kLiteral && !is_long) copy_span_lane(dst + at, src + from, len);
            unsigned long long todo = __ballot(is_long);
            while (todo) {  // uniform in the wave
                const int who = __builtin_ctzll(todo);
                todo &= todo - 1;
                snp_span_wave<false>(dst + __shfl(at, who, 64), src + (uint64_t)__shfl((long long)from, who, 64), __shfl(len, who, 64), lane);
            }
            // copies, in rounds
            const uint32_t off = (uint32_t)from;
            const uint32_t source_end = at - off + (len < off ? len : off);  // a copy that overlaps itself reads up to its own destination
            unsigned long long pending = __ballot(kind == snp::kCopy);
            while (pending) {  // uniform in the wave
                snp_global_order();
                const int first = __builtin_ctzll(pending);
                const uint32_t first_at = __shfl(at, first, 64);
                const bool ready = ((pending >> lane) & 1) && ((int)lane == first || source_end <= first_at);
                if (ready) {
                    uint8_t* d = dst + at;
                    const uint8_t* s = d - off;
                    if (off >= len) {
                        copy_span_lane(d, s, len);
                    } else {
                        for (uint32_t i = 0, j = 0; i < len; ++i) {
                            d[i] = s[j];
                            if (++j == off) j = 0;
                        }
                    }
                }
                pending &= ~__ballot(ready);
            }
            produced = made, cur += pos;
        }
        if (!err && produced != want) err = OXH_SNAPPY_TRUNCATED;
        if (err) {
            snp_global_order();  // the zeros come after what the block stored
            snp_span_wave<true>(dst, nullptr, want, lane);
            ++bad;
        }
        if (lane == 0) status[b] = err;
    }
    if (lane == 0 && bad) atomicAdd(bad_count, bad);
}

__global__ void snappy_clear_kernel(unsigned long long* word) { *word = 0; }

// The kernel over nblocks > 0 blocks, enqueued on st; d_bad: one device word, the blocks with a cause.
int snappy_inflate_enqueue(const uint8_t* d_src, const uint64_t* d_src_lo, const uint64_t* d_src_hi, uint8_t* d_dst, const uint64_t* d_dst_lo,
                           const uint64_t* d_dst_hi, uint32_t* d_status, uint64_t nblocks, unsigned long long* d_bad, hipStream_t st) {
    using namespace oxh::capi;
    snappy_clear_kernel<<<1, 1, 0, st>>>(d_bad);
    HIP_TRY(hipGetLastError());
    const unsigned grid = (unsigned)std::min<uint64_t>(nblocks, snp::kSnappyMaxGroups);
    snappy_inflate_kernel<<<grid, 64, 0, st>>>(d_src, d_src_lo, d_src_hi, d_dst, d_dst_lo, d_dst_hi, d_status, nblocks, d_bad);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

}  // namespace oxh
