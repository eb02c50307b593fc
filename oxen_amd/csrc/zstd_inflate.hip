// oxen_amd/csrc/zstd_inflate.hip -- many Zstandard frames (RFC 8878) inflated per launch (oxh_zstd_inflate_*, and the
// Parquet open's ZSTD pages: parquet_read.hip). The accepted format and the cause codes are stated in
// include/oxen_hash.h "Zstandard"; the entries' checks are capi_dispatch.hip's; the arithmetic on untrusted bytes
// (bit reader, FSE and Huffman tables, section headers, the sequence states) is zstd_tables.hpp's, which the CPU tests.
//
// One wave per frame, workgroups of one wave, a capped grid that loops over the frames: snappy_inflate.hip's shape,
// for the same reason -- a block's entropy streams are found only one symbol from the other, the bytes the sequences
// name are not. Per frame every lane reads the frame header and each block header (the same bytes); a Raw block is a
// whole-wave copy, an RLE block a whole-wave fill. Per Compressed block:
//   prelude  lane 0 reads the literals header, builds the Huffman table (2^11 cells of 2 bytes in LDS) unless the block
//            is treeless, reads the sequence count and the modes, and builds the three FSE tables (2^9, 2^8, 2^9 cells of
//            4 bytes in LDS) that are not Repeat. What it found goes through one record in LDS to the wave. The tables
//            of a frame's earlier block stay where they are for treeless literals and the Repeat mode.
//   literals Huffman streams are decoded a lane a stream (4 lanes, or 1) into the wave's slot: 128 KiB of a scratch the
//            call leases, because the sequences consume them out of order with the matches and a literal's place in
//            the output is not known before its sequence is. (Staging them in the destination's tail was tried on
//            paper: two literal runs of one batch then overlap, source over destination.) Raw literals are read in
//            place, RLE literals are a byte.
//   chase    lane 0 decodes up to 64 sequences from the backward bitstream into cells in LDS (literal source and
//            length, match offset with the repeat offsets resolved, match length, destination). Every cell is checked
//            before it exists: the literals against what the section holds, both lengths against what is left of the
//            frame's size, the offset against 0 < offset <= produced.
//   execute  the whole wave, a cell a lane, as snappy_inflate_kernel does: all literal runs first (256 bytes and more
//            by the whole wave in aligned 16-byte stores), then the matches in rounds -- a match is ready when its source
//            ends at or before the first pending match's destination; a ballot picks them; a workgroup fence between
//            rounds. Unlike Snappy's copies a match may be long (a constant page is one match of 128 KiB): one of 256
//            bytes and more is the whole wave's, also when it overlaps itself.
// The window size is not a limit: the whole output so far is addressable. The content checksum is skipped, not
// verified. A malformed frame sets status[b] to its cause and its whole destination to zeros. No byte outside
// [dst_lo, dst_hi) is written and none outside [src_lo, src_hi) is read; no floating point, no atomics on data.
//
// Changed from the maintainer's sketch, none of it measured against the alternative: the tables are built by one lane
// through the header's builders (the build is short beside the serial decode of a block's literals and sequences, and
// the CPU-tested code is then the code that runs); the grid cap is 512 waves, so the lease is at most 64 MiB.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "snappy_wave.hpp"  // snp_lds_order, snp_global_order, snp_span_wave
#include "zstd_tables.hpp"

namespace oxh {

namespace zs {
constexpr uint32_t kBatch = 64;           // sequences of one chase: a lane each
constexpr uint32_t kLong = 256;           // a literal run or a match of this many bytes and more is the whole wave's
constexpr uint32_t kBlockMax = 1u << 17;  // Block_Maximum_Size; kZstdSlot (capi_internal.hpp) holds a block's literals
static_assert(kZstdSlot == kBlockMax, "a slot is one block's literals");

// What lane 0 found in front of a Compressed block's streams, for the wave; have_* and the logs outlive the block.
struct Prelude {
    uint32_t err;
    uint32_t lit_type, streams, regen, lit_at, stream_n[4], huf_log, have_huf;
    uint32_t nseq, log[3], have[3], bits_at, bits_n;
};

__device__ __forceinline__ uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }

// lane 0: the block blk[0, n) up to its bitstream. Returns 0 or the cause.
__device__ uint32_t prelude(const uint8_t* blk, uint32_t n, Prelude& p, uint16_t* huf, zst::FseCell* t_ll, zst::FseCell* t_of, zst::FseCell* t_ml,
                            uint8_t* weights, uint32_t* work) {
    zst::LitHeader h;
    if (!zst::lit_header(blk, n, h)) return OXH_ZSTD_BLOCK;
    if (h.regen > kBlockMax) return OXH_ZSTD_LITERALS;
    uint32_t at = h.bytes;
    p.lit_type = h.type, p.streams = h.streams, p.regen = h.regen, p.lit_at = at;
    if (h.type < 2) {
        const uint32_t bytes = h.type == 0 ? h.regen : 1;
        if (bytes > n - at) return OXH_ZSTD_BLOCK;
        at += bytes;
    } else {
        if (h.comp > n - at) return OXH_ZSTD_BLOCK;
        uint32_t tree = 0;
        if (h.type == 2) {
            uint32_t count = 0;
            uint32_t rc = zst::huf_read_weights(blk + at, h.comp, weights, &count, &tree, work);
            if (rc == zst::kTabOk) rc = zst::huf_build(weights, count, huf, &p.huf_log, work);
            if (rc) return OXH_ZSTD_LITERALS;
            p.have_huf = 1;
        } else if (!p.have_huf) {
            return OXH_ZSTD_LITERALS;  // treeless, and no block of the frame has left a table
        }
        const uint32_t total = h.comp - tree;  // tree <= comp: huf_read_weights stays inside what it is given
        p.lit_at = at + tree;
        if (h.streams == 1) {
            p.stream_n[0] = total;
        } else {
            if (total < 6) return OXH_ZSTD_LITERALS;
            const uint32_t s1 = le16(blk + p.lit_at), s2 = le16(blk + p.lit_at + 2), s3 = le16(blk + p.lit_at + 4);
            if (6 + s1 + s2 + s3 > total || 3 * ((h.regen + 3) / 4) > h.regen) return OXH_ZSTD_LITERALS;
            p.stream_n[0] = s1, p.stream_n[1] = s2, p.stream_n[2] = s3, p.stream_n[3] = total - 6 - s1 - s2 - s3;
            p.lit_at += 6;
        }
        at += h.comp;
    }
    uint32_t used = 0;
    if (!zst::seq_count(blk + at, n - at, &p.nseq, &used)) return OXH_ZSTD_SEQUENCES;
    at += used;
    if (p.nseq == 0) return at == n ? 0 : OXH_ZSTD_SEQUENCES;
    if (at == n) return OXH_ZSTD_SEQUENCES;
    const uint32_t modes = blk[at++];
    if (modes & 3) return OXH_ZSTD_SEQUENCES;
    int16_t* norm = (int16_t*)work;
    uint16_t* next = (uint16_t*)(norm + zst::kFseSymbols);
    for (uint32_t kind = 0; kind < 3; ++kind) {  // LL, OF, ML: the modes' and the descriptions' order
        zst::FseCell* table = kind == 0 ? t_ll : kind == 1 ? t_of : t_ml;
        const uint32_t max_symbol = kind == 0 ? zst::kMaxLL : kind == 1 ? zst::kMaxOF : zst::kMaxML;
        const uint32_t max_log = kind == 0 ? zst::kLogLL : kind == 1 ? zst::kLogOF : zst::kLogML;
        const uint32_t mode = (modes >> (6 - 2 * kind)) & 3;
        if (mode == 3) {
            if (!p.have[kind]) return OXH_ZSTD_TABLE;
            continue;
        }
        if (mode == 1) {
            if (at == n || blk[at] > max_symbol) return OXH_ZSTD_TABLE;
            table[0] = zst::FseCell{0, blk[at++], 0};
            p.log[kind] = 0;
        } else {
            uint32_t log = 0, rc = 0;
            if (mode == 0) {
                zst::predefined_counts(kind, norm, &log);
            } else {
                rc = zst::fse_read_counts(blk + at, n - at, max_log, max_symbol, norm, &log, &used);
                at += rc ? 0 : used;
            }
            if (rc == zst::kTabOk) rc = zst::fse_build(norm, max_symbol, log, table, next);
            if (rc) return OXH_ZSTD_TABLE;
            p.log[kind] = log;
        }
        p.have[kind] = 1;
    }
    if (at == n) return OXH_ZSTD_SEQUENCES;
    p.bits_at = at, p.bits_n = n - at;
    return 0;
}

// Exactly n bytes of `byte` by the 64 lanes.
__device__ __forceinline__ void fill_wave(uint8_t* dst, uint64_t n, uint8_t byte, unsigned lane) {
    uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    if (lane < head) dst[lane] = byte;
    const uint64_t body = (n - head) & ~15ull, word = 0x0101010101010101ull * byte;
    for (uint64_t b = head + 16ull * lane; b < head + body; b += 16ull * 64) *reinterpret_cast<ulonglong2*>(dst + b) = ulonglong2{word, word};
    if (head + body + lane < n) dst[head + body + lane] = byte;
}

// A match of len bytes at d from d - off, by the 64 lanes; everything it reads lies in front of d.
__device__ __forceinline__ void match_wave(uint8_t* d, uint32_t off, uint32_t len, unsigned lane) {
    const uint8_t* s = d - off;
    if (off >= len) return snp_span_wave<false>(d, s, len, lane);
    uint32_t j = lane % off;
    const uint32_t step = 64 % off;
    for (uint32_t i = lane; i < len; i += 64) {  // d[i] = s[i % off]
        d[i] = s[j];
        j += step;
        if (j >= off) j -= off;
    }
}
}  // namespace zs

// Frame b: src_all[src_lo[b], src_hi[b]) inflates to dst_all[dst_lo[b], dst_hi[b]); status[b] = 0 or the cause;
// bad_count += the frames with a cause. slots: gridDim.x * kZstdSlot bytes.
__global__ __launch_bounds__(64) void zstd_inflate_kernel(const uint8_t* __restrict__ src_all, const uint64_t* __restrict__ src_lo,
                                                          const uint64_t* __restrict__ src_hi, uint8_t* dst_all,
                                                          const uint64_t* __restrict__ dst_lo, const uint64_t* __restrict__ dst_hi,
                                                          uint32_t* __restrict__ status, uint64_t nblocks, uint8_t* slots,
                                                          unsigned long long* __restrict__ bad_count) {
    __shared__ uint16_t huf[zst::kHufCells];
    __shared__ zst::FseCell t_ll[1u << zst::kLogLL], t_of[1u << zst::kLogOF], t_ml[1u << zst::kLogML];
    __shared__ uint8_t weights[256];
    __shared__ uint32_t work[128];  // huf_read_weights' 468 bytes; huf_build's 16 words; norm and next of a sequence table
    __shared__ zs::Prelude pre;
    __shared__ uint32_t cell_lit[zs::kBatch], cell_ll[zs::kBatch], cell_off[zs::kBatch], cell_ml[zs::kBatch], cell_at[zs::kBatch];
    const unsigned lane = threadIdx.x;
    uint8_t* slot = slots + (uint64_t)blockIdx.x * kZstdSlot;
    unsigned long long bad = 0;
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {  // uniform in the wave
        const uint64_t s0 = src_lo[b], s1 = src_hi[b], d0 = dst_lo[b], d1 = dst_hi[b];
        if (s1 < s0 || d1 < d0 || d1 - d0 > 0xFFFFFFFFull || s1 - s0 > 0xFFFFFFFFull) {  // no range to read or to fill, or one past 32 bits
            if (lane == 0) status[b] = OXH_ZSTD_RANGE;
            ++bad;
            continue;
        }
        const uint8_t* src = src_all + s0;
        uint8_t* dst = dst_all + d0;
        const uint64_t n = s1 - s0, want = d1 - d0;
        uint32_t err = 0;
        // ---- the frame header: the same bytes in every lane
        uint64_t cur = 0;
        bool checksum = false;
        if (n < 6) {
            err = n >= 4 && ld32u(src) != 0xFD2FB528u ? OXH_ZSTD_FRAME : OXH_ZSTD_INPUT;
        } else if (ld32u(src) != 0xFD2FB528u) {
            err = OXH_ZSTD_FRAME;  // a skippable frame (184D2A5x) is one of these
        } else {
            const uint32_t fhd = src[4], single = (fhd >> 5) & 1, fcs_flag = fhd >> 6, did_flag = fhd & 3;
            const uint32_t did_bytes = did_flag == 3 ? 4 : did_flag, fcs_bytes = fcs_flag == 0 ? single : 1u << fcs_flag;
            checksum = fhd & 4;
            cur = 5 + (single ? 0 : 1);  // the Window_Descriptor is read over: the whole output is addressable
            if (fhd & 8) {
                err = OXH_ZSTD_FRAME;  // the reserved bit
            } else if (cur + did_bytes + fcs_bytes > n) {
                err = OXH_ZSTD_INPUT;
            } else {
                uint64_t did = 0, fcs = 0;
                for (uint32_t k = 0; k < did_bytes; ++k) did |= (uint64_t)src[cur + k] << (8 * k);
                cur += did_bytes;
                for (uint32_t k = 0; k < fcs_bytes; ++k) fcs |= (uint64_t)src[cur + k] << (8 * k);
                cur += fcs_bytes;
                if (fcs_bytes == 2) fcs += 256;
                if (did)
                    err = OXH_ZSTD_FRAME;  // a dictionary
                else if (fcs_bytes && fcs != want)
                    err = OXH_ZSTD_HEADER;
            }
        }
        snp_lds_order();  // the frame before has read the record
        if (lane == 0) pre.have_huf = 0, pre.have[0] = pre.have[1] = pre.have[2] = 0;
        zst::Repeats reps{1, 4, 8};  // lane 0's are the ones in use
        uint64_t produced = 0;       // below 2^32: want is
        bool last = false;
        while (!err && !last) {
            if (n - cur < 3) {
                err = OXH_ZSTD_INPUT;
                break;
            }
            const uint32_t bh = src[cur] | (uint32_t)src[cur + 1] << 8 | (uint32_t)src[cur + 2] << 16, type = (bh >> 1) & 3, size = bh >> 3;
            last = bh & 1, cur += 3;
            if (type == 3 || size > zs::kBlockMax) {
                err = OXH_ZSTD_BLOCK;
            } else if (type == 0 || type == 1) {  // Raw, RLE
                if ((type == 0 ? size : 1) > n - cur) err = OXH_ZSTD_INPUT;
                else if (size > want - produced) err = OXH_ZSTD_OVERRUN;
                if (err) break;
                if (type == 0) snp_span_wave<false>(dst + produced, src + cur, size, lane);
                else zs::fill_wave(dst + produced, size, src[cur], lane);
                produced += size, cur += type == 0 ? size : 1;
                continue;
            } else if (size > n - cur) {
                err = OXH_ZSTD_INPUT;
            }
            if (err) break;
            // ---- a Compressed block
            const uint8_t* blk = src + cur;
            cur += size;
            snp_lds_order();  // the block before has read the tables and the cells
            if (lane == 0) pre.err = zs::prelude(blk, size, pre, huf, t_ll, t_of, t_ml, weights, work);
            snp_lds_order();
            if ((err = pre.err)) break;
            const uint32_t regen = pre.regen, lit_type = pre.lit_type, nseq = pre.nseq;
            if (regen > want - produced) {
                err = OXH_ZSTD_OVERRUN;
                break;
            }
            const uint8_t* lit = blk + pre.lit_at;  // Raw: the literals; RLE: their byte
            if (lit_type >= 2) {
                bool ok = true;
                if (lane < pre.streams) {
                    const uint32_t per = pre.streams == 4 ? (regen + 3) / 4 : regen;
                    uint32_t from = pre.lit_at;
                    for (uint32_t k = 0; k < lane; ++k) from += pre.stream_n[k];
                    ok = zst::huf_decode_stream(blk + from, pre.stream_n[lane], huf, pre.huf_log, slot + lane * per, lane == 3 ? regen - 3 * per : per);
                }
                if (__ballot(!ok)) {
                    err = OXH_ZSTD_LITERALS;
                    break;
                }
                snp_global_order();  // the slot is read by other lanes than wrote it
                lit = slot;
            }
            const uint8_t rle_byte = lit_type == 1 ? lit[0] : 0;
            // ---- the sequences
            zst::SeqState state{};
            const zst::SeqTables tables{t_ll, t_of, t_ml, pre.log[0], pre.log[1], pre.log[2]};
            uint32_t consumed = 0, done = 0;
            if (nseq && lane == 0 && !zst::seq_open(state, blk + pre.bits_at, pre.bits_n, tables)) err = OXH_ZSTD_SEQUENCES;
            err = __shfl(err, 0, 64);
            while (!err && done < nseq) {
                snp_lds_order();  // the cells before have been read
                uint32_t k = 0, cause = 0;
                uint64_t made = produced;
                if (lane == 0) {
                    while (k < zs::kBatch && done + k < nseq) {
                        uint32_t ll, ml;
                        uint64_t value;
                        zst::seq_next(state, tables, done + k + 1 == nseq, &ll, &ml, &value);
                        const uint64_t off = zst::resolve_offset(reps, value, ll);
                        if (state.b.left < 0 || ll > regen - consumed) cause = OXH_ZSTD_SEQUENCES;
                        else if ((uint64_t)ll + ml > want - made) cause = OXH_ZSTD_OVERRUN;
                        else if (off == 0 || off > made + ll) cause = OXH_ZSTD_OFFSET;
                        if (cause) break;
                        cell_lit[k] = consumed, cell_ll[k] = ll, cell_off[k] = (uint32_t)off, cell_ml[k] = ml, cell_at[k] = (uint32_t)made;
                        consumed += ll, made += (uint64_t)ll + ml, ++k;
                    }
                    if (!cause && done + k == nseq && state.b.left != 0) cause = OXH_ZSTD_SEQUENCES;  // bits no sequence read
                }
                snp_lds_order();
                k = __shfl(k, 0, 64), cause = __shfl(cause, 0, 64), consumed = __shfl(consumed, 0, 64);
                made = (uint64_t)__shfl((long long)made, 0, 64);
                if (cause) {
                    err = cause;
                    break;
                }
                const bool mine = lane < k;
                const uint32_t ll = mine ? cell_ll[lane] : 0, at = mine ? cell_at[lane] : 0, from = mine ? cell_lit[lane] : 0;
                const uint32_t off = mine ? cell_off[lane] : 1, ml = mine ? cell_ml[lane] : 0;
                // literal runs: nothing they read is written here
                const bool long_run = ll >= zs::kLong;
                if (ll && !long_run) {
                    if (lit_type == 1)
                        for (uint32_t i = 0; i < ll; ++i) dst[at + i] = rle_byte;
                    else
                        copy_span_lane(dst + at, lit + from, ll);
                }
                unsigned long long todo = __ballot(long_run);
                while (todo) {  // uniform in the wave
                    const int who = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    uint8_t* to = dst + __shfl(at, who, 64);
                    if (lit_type == 1) zs::fill_wave(to, __shfl(ll, who, 64), rle_byte, lane);
                    else snp_span_wave<false>(to, lit + __shfl(from, who, 64), __shfl(ll, who, 64), lane);
                }
                // matches, in rounds
                const uint32_t m_at = at + ll;
                const uint32_t source_end = m_at - off + (ml < off ? ml : off);  // one that overlaps itself reads up to its own destination
                unsigned long long pending = __ballot(mine);
                while (pending) {  // uniform in the wave
                    snp_global_order();
                    const int first = __builtin_ctzll(pending);
                    const uint32_t first_at = __shfl(m_at, first, 64);
                    const bool ready = ((pending >> lane) & 1) && ((int)lane == first || source_end <= first_at);
                    const bool long_match = ready && ml >= zs::kLong;
                    if (ready && !long_match) {
                        uint8_t* d = dst + m_at;
                        const uint8_t* s = d - off;
                        if (off >= ml) {
                            copy_span_lane(d, s, ml);
                        } else {
                            for (uint32_t i = 0, j = 0; i < ml; ++i) {
                                d[i] = s[j];
                                if (++j == off) j = 0;
                            }
                        }
                    }
                    todo = __ballot(long_match);
                    while (todo) {
                        const int who = __builtin_ctzll(todo);
                        todo &= todo - 1;
                        zs::match_wave(dst + __shfl(m_at, who, 64), __shfl(off, who, 64), __shfl(ml, who, 64), lane);
                    }
                    pending &= ~__ballot(ready);
                }
                produced = made, done += k;
            }
            if (err) break;
            // the literals behind the last sequence
            const uint32_t rest = regen - consumed;
            if (rest > want - produced) {
                err = OXH_ZSTD_OVERRUN;
                break;
            }
            if (lit_type == 1) zs::fill_wave(dst + produced, rest, rle_byte, lane);
            else snp_span_wave<false>(dst + produced, lit + consumed, rest, lane);
            produced += rest;
        }
        if (!err) {
            if (checksum && n - cur < 4) err = OXH_ZSTD_INPUT;
            else if (cur + (checksum ? 4 : 0) != n) err = OXH_ZSTD_FRAME;  // bytes behind the frame: a second frame is not read
            else if (produced != want) err = OXH_ZSTD_TRUNCATED;
        }
        if (err) {
            snp_global_order();  // the zeros come after what the frame stored
            snp_span_wave<true>(dst, nullptr, want, lane);
            ++bad;
        }
        if (lane == 0) status[b] = err;
    }
    if (lane == 0 && bad) atomicAdd(bad_count, bad);
}

__global__ void zstd_clear_kernel(unsigned long long* word) { *word = 0; }

int zstd_inflate_enqueue(const uint8_t* d_src, const uint64_t* d_src_lo, const uint64_t* d_src_hi, uint8_t* d_dst, const uint64_t* d_dst_lo,
                         const uint64_t* d_dst_hi, uint32_t* d_status, uint64_t nblocks, uint8_t* d_slots, unsigned long long* d_bad, hipStream_t st) {
    using namespace oxh::capi;
    zstd_clear_kernel<<<1, 1, 0, st>>>(d_bad);
    HIP_TRY(hipGetLastError());
    zstd_inflate_kernel<<<zstd_grid(nblocks), 64, 0, st>>>(d_src, d_src_lo, d_src_hi, d_dst, d_dst_lo, d_dst_hi, d_status, nblocks, d_slots, d_bad);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

}  // namespace oxh
