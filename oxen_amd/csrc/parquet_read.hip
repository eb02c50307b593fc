// oxen_amd/csrc/parquet_read.hip -- the bytes of an uncompressed or SNAPPY, flat Parquet file in HBM to a page index and to
// typed Arrow columns (oxh_parquet_*): what read_df_parquet / scan_parquet (core/df/tabular.rs:111, :172) are for.
// The format and the refusals are stated in include/oxen_hash.h "Parquet: the file's bytes"; the varint, the Thrift
// reader, the PageHeader, the hybrid's run header and the bit extraction are parquet_bits.hpp's, the code
// tests/native/parquet_read_host_test.cpp runs on the host; the footer's plan and the page table's checks are
// parquet_read_host.hpp's; the column entries' checks are csv_host.hpp's.
//
// Open: the footer comes down and becomes a plan (host). pq_walk_kernel, one lane per column chunk, chases the
// chunk's PageHeaders -- each is found only from the one before -- first counting, then filling one fixed record per
// page. The table comes down; the host checks it and lists every column's data and dictionary pages with their row
// and word bases (a prefix over the table), which is all the column kernels read of the file's structure.
// With OXH_PARQUET_INFLATE the walk also takes the pages of SNAPPY chunks, whose sizes differ; between the table's
// checks and the page lists, inflate_pages gives every compressed page a place in an image the handle owns, copies a
// V2 page's stored levels there (pq_stored_kernel), inflates the rest (snappy_inflate.hip, the kernel of
// oxh_snappy_inflate_*) and reads the V1 pages' level lengths out of the inflated bodies (pq_level_length_kernel). A
// page's body is from then on in the file or in the image: pq_body / pq_at are the column kernels' only way to it.
// Columns, per selected column, on one stream (launches order the steps, no workgroup waits for another):
//   levels   pq_levels_kernel, a wave per data page of an OPTIONAL column: the run headers are chased by the whole
//            wave (uniform control flow, every lane reads the same header), a run's bits are expanded by the 64 lanes
//            into page-local validity words that start on a word, with the valid rows in front of every word and the
//            page's valid count. An RLE run costs no load. A REQUIRED column has no such pass;
//   indices  pq_index_kernel, a wave per dictionary-coded page (width w = the values' first byte) and per page of RLE
//            booleans (width 1): the same chase, lanes extract value k at bit k * w into a u32 per value rank. An
//            index at or beyond the dictionary's size becomes 0 before any load and sets the error word;
//   gather   pq_fixed_kernel / pq_bool_kernel, a lane per OUTPUT row: its page by a search of the page list, its
//            validity bit and rank from the page's words, the value from the PLAIN body at rank * width (any
//            alignment) or from dict[index[rank]], stored coalesced at out[row], widened in the store; a null's slot
//            is 0. Booleans and the validity bitmap leave as ballots, 8 bytes a wave, so pages of 100 rows that share
//            a byte still have one writer per byte;
//   strings  pq_chase_kernel, a wave per PLAIN page and per dictionary page: the length chain is serial, so the wave
//            loads the body through LDS in 1 KiB windows, one lane chases `4 + length` inside the window into up to
//            64 (offset, length) cells, and the wave stores them by rank. A length that leaves the page sets the error
//            word and ends the page. pq_strlen_kernel, a lane per row, gives every row its source and length (a null
//            0); exclusive_scan_u32 gives the offsets, its total the measure's value bytes; pq_strcopy_kernel copies,
//            a cell of 512 bytes and more by the whole wave.
// List columns (repetition levels) are parquet_lists.hip's, over the same handle (parquet_read_device.hpp).
// One writer per output byte; scratch that a malformed page cuts short is filled with zeros, so no result depends on
// what scratch or the outputs held; every load is bounded by the page, run or window it belongs to.
#include "parquet_read_device.hpp"

using namespace oxh::capi;

namespace oxh {

namespace pqr {
constexpr uint32_t kWindow = 1024;  // bytes of a page the chase looks at at once: 64 lanes x 16
constexpr uint32_t kLongCell = csv::kLongCell;
}  // namespace pqr

__device__ __forceinline__ void pq_wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------- open: the page walk
// FILL false: counts[ch] = the pages of chunk ch. FILL true: its records at recs[page0 ..].
template <bool FILL>
__global__ __launch_bounds__(64) void pq_walk_kernel(const uint8_t* __restrict__ bytes, const pqr::ChunkDesc* __restrict__ chunks, uint64_t nchunks,
                                                     uint32_t* __restrict__ counts, pqr::PageRec* __restrict__ recs,
                                                     unsigned long long* __restrict__ ctrl) {
    __shared__ uint64_t skip_words[64][pqr::kSkipDepth];  // a lane's open containers while it skips a field: LDS, not scratch
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; ch < nchunks; ch += stride) {
        const pqr::ChunkDesc c = chunks[ch];
        uint64_t pos = 0, seen = 0;
        uint32_t n = 0;
        bool bad = false;
        while (pos < c.bytes && seen < c.num_values) {
            pqr::Span s{bytes + c.at + pos, c.bytes - pos, 0, false};
            pqr::PageInfo h;
            if (!pqr::page_header(s, h, skip_words[threadIdx.x]) || h.csize < 0 || h.usize < 0 || h.num_values < 0 || (uint64_t)h.csize > s.n - s.at) {
                bad = true;
                break;
            }
            const uint64_t body = pos + s.at;
            const bool data = h.type == pqr::kPageData || h.type == pqr::kPageDataV2;
            // a SNAPPY or ZSTD chunk compresses every page this reader reads, but a V2 page that says it is stored
            const bool packed = c.codec != pqr::kCodecNone && (h.type == pqr::kPageData || h.type == pqr::kPageDict || (h.type == pqr::kPageDataV2 && h.is_compressed));
            if (!packed && h.csize != h.usize && (data || h.type == pqr::kPageDict || c.codec == pqr::kCodecNone)) {
                bad = true;
                break;
            }
            const uint32_t size = (uint32_t)(packed ? h.usize : h.csize);  // of the body the column kernels read
            pqr::PageRec r{c.at + body, size, (uint32_t)h.type, (uint32_t)h.num_values, (uint32_t)h.encoding, 0, 0, 0, packed ? pqr::kPageInImage | (c.codec == pqr::kCodecZstd ? pqr::kPageZstd : 0u) : 0u,
                           (uint32_t)h.csize, 0};
            if (h.type == pqr::kPageData && c.optional) {  // V1: the levels' 4-byte length leads the body
                if (size < 4) {
                    bad = true;
                    break;
                }
                if (packed)
                    r.flags |= pqr::kPageLevelsLater;  // the inflated body's: the open finishes the record
                else
                    pqr::finish_v1_levels(r, pqr::le32(bytes + c.at + body));
                // a list's chunk (optional == 2): the length read here is its repetition stream's (pqr::ListPage)
                if (h.def_enc != pqr::kEncRle || (c.optional == 2 && h.rep_enc != pqr::kEncRle)) r.flags |= 2;
            } else if (h.type == pqr::kPageDataV2) {
                if (h.rep_len < 0 || h.def_len < 0) {
                    bad = true;
                    break;
                }
                const uint64_t levels = (uint64_t)h.rep_len + (uint64_t)h.def_len;
                r.def_at = (uint32_t)h.rep_len, r.def_bytes = c.optional ? (uint32_t)h.def_len : 0;
                r.values_at = levels <= (uint64_t)h.csize && levels <= size ? (uint32_t)levels : ~0u;  // the host refuses it
                if (packed) r.stored = r.values_at != ~0u ? (uint32_t)levels : 0;
                if (h.rep_len) r.flags |= 1;
            }
            if (FILL) {
                if (n >= counts[ch]) {  // the buffer changed between the passes
                    bad = true;
                    break;
                }
                recs[c.page0 + n] = r;
            }
            if (data) seen += (uint64_t)h.num_values;
            pos = body + (uint64_t)h.csize;
            ++n;
        }
        if (seen != c.num_values) bad = true;
        if (!FILL) counts[ch] = n;
        if (FILL && n != counts[ch]) bad = true;
        if (bad) atomicMax(&ctrl[0], (unsigned long long)ch + 1);  // the last chunk that failed, + 1
    }
}

// ---------------------------------------------------------------- columns
__device__ __forceinline__ uint32_t pq_find_page(const PqColumn& c, uint64_t row) {  // the last page whose row0 <= row
    uint32_t lo = 0, hi = c.npages;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (c.pages[mid].row0 <= row)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The row's page, whether it holds a value, and the value's rank among its page's values.
__device__ __forceinline__ bool pq_row(const PqColumn& c, uint64_t row, uint32_t& page, uint32_t& rank) {
    page = pq_find_page(c, row);
    const pqr::DataPage& pg = c.pages[page];
    const uint64_t local = row - pg.row0;
    if (local >= pg.num_values) return rank = 0, false;  // the host's prefix says it cannot happen
    if (!c.optional) return rank = (uint32_t)local, true;
    const uint64_t w = c.words[pg.word0 + (local >> 6)];
    rank = c.prefix[pg.word0 + (local >> 6)] + (uint32_t)__popcll(w & ((1ull << (local & 63)) - 1));
    return (w >> (local & 63)) & 1;
}

__global__ __launch_bounds__(256) void pq_levels_kernel(const PqColumn c, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long nulls = 0, bad = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < c.npages; p += (uint64_t)gridDim.x * 4) {  // uniform in the wave
        const pqr::DataPage pg = c.pages[p];
        const uint64_t n = pg.num_values, nwords = (n + 63) / 64;
        uint64_t* words = c.words + pg.word0;
        uint32_t* prefix = c.prefix + pg.word0;
        pqr::Span s{pq_body(c, pg) + pg.def_at, pg.def_bytes, 0, false};
        uint64_t pos = 0, acc = 0;
        uint32_t running = 0;
        bool ok = true;
        while (pos < n && ok) {
            pqr::Run r;
            if (!pqr::next_run(s, 1, n - pos, r)) {
                ok = false;
                break;
            }
            const uint64_t take = r.count < n - pos ? r.count : n - pos;
            for (uint64_t done = 0; done < take;) {
                const uint64_t room = 64 - (pos & 63), len = take - done < room ? take - done : room;
                uint64_t bits;
                if (r.packed)
                    bits = __ballot(lane < len && pqr::extract(r.body, r.avail, done + lane, 1));
                else
                    bits = r.value ? (len == 64 ? ~0ull : (1ull << len) - 1) : 0;
                acc |= bits << (pos & 63);
                pos += len, done += len;
                if ((pos & 63) == 0) {
                    if (lane == 0) words[(pos >> 6) - 1] = acc, prefix[(pos >> 6) - 1] = running;
                    running += (uint32_t)__popcll(acc), acc = 0;
                }
            }
        }
        // the last word, and after a malformed stream every word it did not reach: nulls
        for (uint64_t w = pos >> 6; w < nwords; ++w) {
            if (lane == 0) words[w] = acc, prefix[w] = running;
            running += (uint32_t)__popcll(acc), acc = 0;
        }
        if (lane == 0) c.page_valid[p] = running;
        nulls += n - running;
        if (!ok) bad |= pqr::kErrLevels;
    }
    if (lane == 0) {
        if (nulls) atomicAdd(&ctrl[pqr::kColNulls], nulls);
        if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void pq_index_kernel(const PqColumn c, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long coded = 0, bad = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < c.npages; p += (uint64_t)gridDim.x * 4) {  // uniform in the wave
        const pqr::DataPage pg = c.pages[p];
        const bool dict = pg.dict != ~0u;
        if (!dict && pg.encoding != (uint32_t)pqr::kEncRle) continue;
        const uint64_t nvalid = c.optional ? c.page_valid[p] : pg.num_values;
        const uint8_t* v = pq_body(c, pg) + pg.values_at;
        const uint64_t nb = pg.body_size - pg.values_at;
        uint32_t* out = c.idx + pg.row0;
        pqr::Span s{v, 0, 0, false};
        uint32_t w = 1, limit = 2;
        bool ok = true;
        if (dict) {  // the width, then the runs
            limit = c.dicts[pg.dict].num_values;
            if (nb < 1 || v[0] > 32)
                ok = false;
            else
                w = v[0], s.p = v + 1, s.n = nb - 1;
        } else {  // RLE booleans: the runs' length, then the runs
            if (nb < 4 || pqr::le32(v) > nb - 4)
                ok = false;
            else
                s.p = v + 4, s.n = pqr::le32(v);
        }
        uint64_t pos = 0;
        while (pos < nvalid && ok) {
            pqr::Run r;
            if (!pqr::next_run(s, w, nvalid - pos, r)) {
                ok = false;
                break;
            }
            const uint64_t take = r.count < nvalid - pos ? r.count : nvalid - pos;
            bool beyond = false;
            for (uint64_t j = lane; j < take; j += 64) {
                uint32_t k = r.packed ? pqr::extract(r.body, r.avail, j, w) : r.value;
                if (k >= limit) k = 0, beyond = true;  // never an index outside the dictionary
                out[pos + j] = k;
            }
            if (__ballot(beyond)) bad |= pqr::kErrIndex;
            pos += take;
        }
        for (uint64_t j = pos + lane; j < nvalid; j += 64) out[j] = 0;  // what a malformed stream did not reach
        if (!ok) bad |= pqr::kErrIndex;
        if (dict) coded += nvalid;
    }
    if (lane == 0) {
        if (coded) atomicAdd(&ctrl[pqr::kColDictValues], coded);
        if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// SRC: the bytes of a value in the file; DST: of a cell of `values`; a 4 -> 8 store sign-extends an integer and
// widens a float exactly.
template <uint32_t SRC, uint32_t DST, bool FLOAT>
__global__ __launch_bounds__(256) void pq_fixed_kernel(const PqColumn c, void* __restrict__ values, uint8_t* __restrict__ validity,
                                                       unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = c.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballot
    bool bad = false;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool valid = false;
        if (i < n) {
            uint32_t page, rank;
            valid = pq_row(c, i, page, rank);
            uint64_t out = 0;
            if (valid) {
                const uint8_t* src = pq_fixed_source<SRC>(c, c.pages[page], rank, bad);
                if (src) {
                    if (SRC == 8) {
                        out = ld64u(src);
                    } else if (DST == 4) {
                        out = ld32u(src);
                    } else if (FLOAT) {
                        out = (uint64_t)__double_as_longlong((double)__uint_as_float(ld32u(src)));
                    } else {
                        out = (uint64_t)(int64_t)(int32_t)ld32u(src);
                    }
                }
            }
            if (DST == 8)
                ((uint64_t*)values)[i] = out;
            else
                ((uint32_t*)values)[i] = (uint32_t)out;
        }
        pq_store_word(validity, __ballot(valid), i - lane, n, lane);
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], pqr::kErrValues, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void pq_bool_kernel(const PqColumn c, uint8_t* __restrict__ bits, uint8_t* __restrict__ validity,
                                                      unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = c.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    bool bad = false;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool valid = false, truth = false;
        if (i < n) {
            uint32_t page, rank;
            valid = pq_row(c, i, page, rank);
            const pqr::DataPage& pg = c.pages[page];
            if (valid && pg.encoding == (uint32_t)pqr::kEncRle) {
                truth = c.idx[pg.row0 + rank] & 1;
            } else if (valid) {
                const uint64_t at = (uint64_t)pg.values_at + (rank >> 3);
                if (at < pg.body_size)
                    truth = (pq_body(c, pg)[at] >> (rank & 7)) & 1;
                else
                    bad = true;
            }
        }
        pq_store_word(bits, __ballot(truth), i - lane, n, lane);
        pq_store_word(validity, __ballot(valid), i - lane, n, lane);
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], pqr::kErrValues, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// DICT false: a wave per PLAIN data page; DICT true: per dictionary page. The cells (where each starts in its page's
// body, its length) by rank.
template <bool DICT>
__global__ __launch_bounds__(256) void pq_chase_kernel(const PqColumn c, unsigned long long* __restrict__ ctrl) {
    __shared__ uint8_t win_all[4][pqr::kWindow];
    __shared__ uint32_t at_all[4][64], len_all[4][64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* win = win_all[wave];
    uint32_t *cat = at_all[wave], *clen = len_all[wave];
    const uint64_t njobs = DICT ? c.ndicts : c.npages;
    unsigned long long bad = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + wave; p < njobs; p += (uint64_t)gridDim.x * 4) {  // uniform in the wave
        const uint8_t* body;
        uint64_t first, nb, count;
        uint32_t *out_at, *out_len;
        if (DICT) {
            const pqr::DictPage d = c.dicts[p];
            body = pq_body(c, d), first = 0, nb = d.body_size, count = d.num_values;
            out_at = c.dict_at + d.entry0, out_len = c.dict_len + d.entry0;
        } else {
            const pqr::DataPage pg = c.pages[p];
            if (pg.dict != ~0u) continue;
            body = pq_body(c, pg), first = pg.values_at, nb = pg.body_size, count = c.optional ? c.page_valid[p] : pg.num_values;
            out_at = c.cell_at + pg.row0, out_len = c.cell_len + pg.row0;
        }
        uint64_t cur = first, done = 0;  // the same in every lane
        bool ok = true;
        while (done < count && ok) {
            const uint32_t wlen = (uint32_t)(nb - cur < pqr::kWindow ? nb - cur : pqr::kWindow);
            pq_wave_lds_order();  // the window before has been read
            if (16 * lane + 16 <= wlen) {
                const uint64_t a = ld64u(body + cur + 16 * lane), b = ld64u(body + cur + 16 * lane + 8);
                __builtin_memcpy(win + 16 * lane, &a, 8);
                __builtin_memcpy(win + 16 * lane + 8, &b, 8);
            } else {
                for (uint32_t k = 16 * lane; k < wlen && k < 16 * lane + 16; ++k) win[k] = body[cur + k];
            }
            pq_wave_lds_order();
            uint32_t k = 0;
            uint64_t pos = 0;
            if (lane == 0) {
                while (k < 64 && done + k < count && pos + 4 <= wlen) {
                    const uint32_t len = pqr::le32(win + pos);
                    const uint64_t at = cur + pos + 4;
                    if (len > nb - at) break;  // the chain leaves the page
                    cat[k] = (uint32_t)at, clen[k] = len, ++k;
                    pos += 4 + (uint64_t)len;
                }
            }
            pq_wave_lds_order();
            k = __shfl(k, 0, 64);
            pos = (uint64_t)__shfl((long long)pos, 0, 64);
            if (k == 0) {  // no whole cell where one is due
                ok = false;
                break;
            }
            if (lane < k) out_at[done + lane] = cat[lane], out_len[done + lane] = clen[lane];
            done += k, cur += pos;
        }
        for (uint64_t j = done + lane; j < count; j += 64) out_at[j] = 0, out_len[j] = 0;  // what a broken chain did not reach
        if (!ok) bad |= pqr::kErrChain;
    }
    if (lane == 0 && bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lens[i] / src[i] (both may be NULL: the measure) = the bytes of row i's string and where they start in the file;
// validity (may be NULL); ctrl: the bytes.
__global__ __launch_bounds__(256) void pq_strlen_kernel(const PqColumn c, uint32_t* __restrict__ lens, uint64_t* __restrict__ src,
                                                        uint8_t* __restrict__ validity, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = c.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballot
    unsigned long long bytes = 0;
    bool bad = false;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool valid = false;
        uint32_t len = 0;
        uint64_t from = 0;
        if (i < n) {
            uint32_t page, rank;
            valid = pq_row(c, i, page, rank);
            const pqr::DataPage& pg = c.pages[page];
            if (valid && pg.dict != ~0u) {
                const pqr::DictPage& d = c.dicts[pg.dict];
                const uint32_t k = c.idx[pg.row0 + rank];
                if (k < d.num_values)
                    len = c.dict_len[d.entry0 + k], from = pq_place(d, c.dict_at[d.entry0 + k]);
                else
                    bad = true;  // an empty dictionary
            } else if (valid) {
                len = c.cell_len[pg.row0 + rank], from = pq_place(pg, c.cell_at[pg.row0 + rank]);
            }
            if (lens) lens[i] = len, src[i] = from;
        }
        pq_store_word(validity, __ballot(valid), i - lane, n, lane);
        unsigned long long sum = len;
#pragma unroll
        for (int off = 32; off; off >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, off, 64);
        bytes += sum;
    }
    if (lane == 0 && bytes) atomicAdd(&ctrl[pqr::kColBytes], bytes);
    if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], pqr::kErrValues, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (lens are written and scanned into starts) offsets[0 .. n] and the bytes of every string.
__global__ __launch_bounds__(256) void pq_strcopy_kernel(const PqColumn c, const uint32_t* __restrict__ lens, const uint64_t* __restrict__ src,
                                                         const uint64_t* __restrict__ starts, uint64_t total, void* __restrict__ offsets, uint32_t wide,
                                                         uint8_t* __restrict__ values, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = c.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: the long cells are a whole wave's
    unsigned long long bad = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        uint64_t at = 0, from = 0;
        uint32_t len = 0;
        if (i < n) {
            at = starts[i], len = lens[i], from = src[i];
            if (at + len > total) bad |= pqr::kErrPlace, len = 0;  // never a store outside the total bytes
            if (wide) {
                ((uint64_t*)offsets)[i] = at;
                if (i + 1 == n) ((uint64_t*)offsets)[n] = total;
            } else {
                ((uint32_t*)offsets)[i] = (uint32_t)at;
                if (i + 1 == n) ((uint32_t*)offsets)[n] = (uint32_t)total;
            }
        }
        const bool is_long = len >= pqr::kLongCell;
        if (len && !is_long) copy_span_lane(values + at, pq_at(c, from), len);
        unsigned long long todo = __ballot(is_long);
        while (todo) {  // uniform in the wave
            const int who = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint8_t* p = pq_at(c, (uint64_t)__shfl((long long)from, who, 64));
            uint8_t* d = values + (uint64_t)__shfl((long long)at, who, 64);
            copy_span_wave(d, p, __shfl(len, who, 64), lane);
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[pqr::kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- open: the compressed pages
// A wave per compressed V2 page: its levels, stored as they are in front of the compressed values, to the front of
// its body in the image. jobs[3 j ..] = {where in the file, where in the image, bytes}.
__global__ __launch_bounds__(256) void pq_stored_kernel(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ image, const uint64_t* __restrict__ jobs,
                                                        uint64_t njobs) {
    const unsigned lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < njobs; j += (uint64_t)gridDim.x * 4)
        copy_span_wave(image + jobs[3 * j + 1], bytes + jobs[3 * j], jobs[3 * j + 2], lane);
}

// A lane per compressed V1 page of an OPTIONAL column: out[j] = the first 4 bytes of its inflated body, the
// levels' length. at[j]: the body in the image (at least 4 bytes: the walk checked).
__global__ __launch_bounds__(256) void pq_level_length_kernel(const uint8_t* __restrict__ image, const uint64_t* __restrict__ at, uint64_t n,
                                                              uint32_t* __restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) out[j] = pqr::le32(image + at[j]);
}

// Device words to zero (a captured graph takes no memset; neither does this file).
__global__ __launch_bounds__(256) void pq_clear_kernel(unsigned long long* __restrict__ words, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) words[i] = 0;
}

int pq_index_enqueue(const PqColumn& c, unsigned long long* d_ctrl, hipStream_t st) {
    pq_index_kernel<<<pq_wave_grid(c.npages), 256, 0, st>>>(c, d_ctrl);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

int pq_clear_enqueue(unsigned long long* d_words, uint64_t n, hipStream_t st) {
    pq_clear_kernel<<<pq_cap_grid((n + 255) / 256), 256, 0, st>>>(d_words, n);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

}  // namespace oxh

namespace {

namespace csv = oxh::csv;
namespace pqr = oxh::pqr;
using oxh::PqColumn;

using oxh::ParquetHandle;

unsigned cap_grid(uint64_t groups) { return oxh::pq_cap_grid(groups); }
unsigned row_grid(uint64_t n) { return oxh::pq_row_grid(n); }
unsigned wave_grid(uint64_t jobs) { return oxh::pq_wave_grid(jobs); }
ParquetHandle* handle_of(void* p) { return oxh::pq_handle_of(p); }
int device_enter(oxh_ctx* ctx) { return oxh::pq_device_enter(ctx); }

void take_footer(ParquetHandle& h, pqr::Footer&& f) {
    h.footer = std::move(f);
    h.name_offsets.assign(1, 0);
    for (const pqr::Leaf& leaf : h.footer.leaves) {
        h.names.insert(h.names.end(), leaf.name.begin(), leaf.name.end());
        h.name_offsets.push_back(h.names.size());
    }
}

const char* snappy_cause(uint32_t code) {
    static const char* names[] = {"", "its preamble is not the page's uncompressed size", "a tag or a literal leaves the page", "a copy with offset 0",
                                  "a copy from in front of the page's first byte", "an element passes the page's uncompressed size",
                                  "the stream ends before the page's uncompressed size", "its range is not one"};
    return code < 8 ? names[code] : "an unknown cause";
}
const char* zstd_cause(uint32_t code) {
    static const char* names[] = {"", "not a frame this reader reads (magic, dictionary, reserved bit, bytes behind it)",
                                  "its content size is not the page's uncompressed size", "the frame leaves the page", "a block or one of its sections is malformed",
                                  "Huffman literals are malformed", "an FSE table is malformed", "a sequence bitstream is malformed",
                                  "an offset of 0 or from in front of the page's first byte", "the frame passes the page's uncompressed size",
                                  "the frame ends before the page's uncompressed size", "its range is not one"};
    return code < 12 ? names[code] : "an unknown cause";
}

// Every compressed page of the table inflated into an image the handle owns, and the records that need the inflated
// body finished: a record's body is then its place in the image. `lease`: the open's, whose walk is over.
int inflate_pages(ParquetHandle& h, const std::vector<pqr::ChunkDesc>& chunks, const std::vector<uint32_t>& counts, std::vector<pqr::PageRec>& recs,
                  oxh::ScratchLease& lease, hipStream_t st) {
    using namespace oxh;
    const uint64_t ncols = h.ncols();
    auto where = [&](uint64_t page) {  // the chunk of a record
        uint64_t ch = 0;
        while (ch + 1 < chunks.size() && !(chunks[ch].page0 <= page && page - chunks[ch].page0 < counts[ch])) ++ch;
        return "row group " + std::to_string(ch / ncols) + ", column '" + h.footer.leaves[ch % ncols].name + "'";
    };
    const pqr::ImagePlan plan = pqr::plan_image(recs);
    if (plan.implausible != ~0ull) {
        const pqr::PageRec& r = recs[plan.implausible];
        return fail(OXH_ERR_INVALID, "parquet open: " + where(plan.implausible) + ": a page of " + std::to_string(r.file_size) + " compressed bytes claims " +
                                         std::to_string(r.body_size) + " uncompressed ones, more than any " +
                                         (r.flags & pqr::kPageZstd ? "Zstandard frame gives (128 KiB per 3 bytes behind the header)" : "Snappy stream gives (22 x + 32)"));
    }
    if (!plan.pages) return OXH_OK;
    // the blocks, the stored levels and the V1 pages whose level length is in the inflated body
    std::vector<uint64_t> tables, stored, later;
    std::vector<uint64_t> block_page, zstd_page;  // the SNAPPY pages; the ZSTD pages go behind them: a launch per codec
    for (size_t k = 0; k < recs.size(); ++k) {
        const pqr::PageRec& r = recs[k];
        if (!(r.flags & pqr::kPageInImage)) continue;
        (r.flags & pqr::kPageZstd ? zstd_page : block_page).push_back(k);
        if (r.stored) stored.insert(stored.end(), {r.body, plan.places[k], (uint64_t)r.stored});
    }
    const uint64_t nsnappy = block_page.size(), nzstd = zstd_page.size();
    block_page.insert(block_page.end(), zstd_page.begin(), zstd_page.end());
    for (uint64_t k : block_page)  // in the blocks' order: the lengths come back in it
        if (recs[k].flags & pqr::kPageLevelsLater) later.push_back(plan.places[k]);
    const uint64_t nb = block_page.size(), nstored = stored.size() / 3, nlater = later.size();
    tables.resize(4 * nb);  // src_lo | src_hi | dst_lo | dst_hi
    for (uint64_t j = 0; j < nb; ++j) {
        const pqr::PageRec& r = recs[block_page[j]];
        tables[j] = r.body + r.stored, tables[nb + j] = r.body + r.file_size;
        tables[2 * nb + j] = plan.places[block_page[j]] + r.stored, tables[3 * nb + j] = plan.places[block_page[j]] + r.body_size;
    }
    if (hipMalloc(&h.image, plan.bytes) != hipSuccess) {
        (void)hipGetLastError();
        h.image = nullptr;
        return fail(OXH_ERR_NOMEM, "parquet open: " + std::to_string(plan.bytes) + " B for the inflated pages on the device");
    }
    h.image_bytes = plan.bytes;
    poison_device(h.image, plan.bytes, st);
    csv::Carver carve;
    const uint64_t at_bad = carve(16), at_slots = carve(nzstd ? zstd_slot_bytes(nzstd) : 0), at_tables = carve(tables.size() * 8), at_status = carve(nb * 4), at_stored = carve(stored.size() * 8),
                   at_later = carve(nlater * 8), at_lengths = carve(nlater * 4);
    void* lbase = nullptr;
    if (lease.get(carve.at, &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet open: " + std::to_string(carve.at) + " B of block tables for the inflation");
    }
    uint8_t* b = (uint8_t*)lbase;
    const uint64_t* d_tables = (const uint64_t*)(b + at_tables);
    std::vector<uint32_t> status(nb), lengths(nlater);
    unsigned long long bad[2] = {0, 0};
    int rc = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(b + at_tables, tables.data(), tables.size() * 8, hipMemcpyHostToDevice, st));
        if (nstored) {
            HIP_TRY(hipMemcpyAsync(b + at_stored, stored.data(), stored.size() * 8, hipMemcpyHostToDevice, st));
            pq_stored_kernel<<<wave_grid(nstored), 256, 0, st>>>(h.d_bytes, h.image, (const uint64_t*)(b + at_stored), nstored);
            HIP_TRY(hipGetLastError());
        }
        int r = OXH_OK;
        if (nsnappy)
            r = snappy_inflate_enqueue(h.d_bytes, d_tables, d_tables + nb, h.image, d_tables + 2 * nb, d_tables + 3 * nb, (uint32_t*)(b + at_status), nsnappy,
                                       (unsigned long long*)(b + at_bad), st);
        if (r) return r;
        if (nzstd)
            r = zstd_inflate_enqueue(h.d_bytes, d_tables + nsnappy, d_tables + nb + nsnappy, h.image, d_tables + 2 * nb + nsnappy, d_tables + 3 * nb + nsnappy,
                                     (uint32_t*)(b + at_status) + nsnappy, nzstd, b + at_slots, (unsigned long long*)(b + at_bad) + 1, st);
        if (r) return r;
        if (nlater) {
            HIP_TRY(hipMemcpyAsync(b + at_later, later.data(), nlater * 8, hipMemcpyHostToDevice, st));
            pq_level_length_kernel<<<row_grid(nlater), 256, 0, st>>>(h.image, (const uint64_t*)(b + at_later), nlater, (uint32_t*)(b + at_lengths));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(lengths.data(), b + at_lengths, nlater * 4, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(status.data(), b + at_status, nb * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(bad, b + at_bad, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) return (void)hipStreamSynchronize(st), rc;
    for (uint64_t j = 0; j < nb; ++j)
        if (status[j])
            return fail(OXH_ERR_INVALID, "parquet open: " + where(block_page[j]) + (j < nsnappy ? ": a page's Snappy stream is malformed: " + std::string(snappy_cause(status[j]))
                                                                                                : ": a page's Zstandard frame is malformed: " + std::string(zstd_cause(status[j]))));
    if ((nsnappy && bad[0]) || (nzstd && bad[1])) return fail(OXH_ERR_HIP, "parquet open: the inflation counts a malformed page and names none");
    uint64_t nth = 0;
    for (uint64_t j = 0; j < nb; ++j) {
        pqr::PageRec& r = recs[block_page[j]];
        r.body = plan.places[block_page[j]];
        if (r.flags & pqr::kPageLevelsLater) pqr::finish_v1_levels(r, lengths[nth++]);
    }
    h.pages_inflated = nb;
    return OXH_OK;
}

// The page walk over h->d_bytes and every column's page lists; stats8 is filled on success.
int open_run(ParquetHandle& h, uint64_t* stats8, hipStream_t st) {
    using namespace oxh;
    const pqr::Footer& f = h.footer;
    const uint64_t ncols = h.ncols(), nchunks = f.chunks.size();
    std::vector<pqr::ChunkDesc> chunks(nchunks);
    for (uint64_t k = 0; k < nchunks; ++k)
        chunks[k] = pqr::ChunkDesc{f.chunks[k].at, f.chunks[k].bytes, f.chunks[k].num_values, f.leaves[k % ncols].list ? 2u : f.leaves[k % ncols].required ? 0u : 1u,
                                   0, f.chunks[k].codec, 0};
    std::vector<uint32_t> counts(nchunks, 0);
    std::vector<pqr::PageRec> recs;
    if (nchunks) {
        ScratchLease lease(st);
        void* lbase = nullptr;
        csv::Carver carve;
        const uint64_t at_ctrl = carve(csv::kCtrlBytes), at_chunks = carve(nchunks * sizeof(pqr::ChunkDesc)), at_counts = carve(nchunks * 4);
        if (lease.get(carve.at, &lbase) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "parquet open: " + std::to_string(carve.at) + " B of chunk descriptors and page counts");
        }
        uint8_t* b = (uint8_t*)lbase;
        unsigned long long* d_ctrl = (unsigned long long*)(b + at_ctrl);
        pqr::ChunkDesc* d_chunks = (pqr::ChunkDesc*)(b + at_chunks);
        uint32_t* d_counts = (uint32_t*)(b + at_counts);
        pqr::PageRec* d_recs = nullptr;
        const unsigned grid = cap_grid((nchunks + 63) / 64);
        unsigned long long err = 0;
        int rc = [&]() -> int {
            pq_clear_kernel<<<1, 256, 0, st>>>(d_ctrl, csv::kCtrlBytes / 8);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), nchunks * sizeof(pqr::ChunkDesc), hipMemcpyHostToDevice, st));
            pq_walk_kernel<false><<<grid, 64, 0, st>>>(h.d_bytes, d_chunks, nchunks, d_counts, nullptr, d_ctrl);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, nchunks * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&err, d_ctrl, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (err) return OXH_OK;
            uint64_t total = 0;
            for (uint64_t k = 0; k < nchunks; ++k) {
                if (total > 0xFFFFFFFFull) return fail(OXH_ERR_INVALID, "parquet open: more than 2^32 pages");
                chunks[k].page0 = (uint32_t)total, total += counts[k];
            }
            if (!total) return OXH_OK;
            recs.resize(total);
            if (hipMalloc(&d_recs, total * sizeof(pqr::PageRec)) != hipSuccess) {
                (void)hipGetLastError();
                d_recs = nullptr;
                return fail(OXH_ERR_NOMEM, "parquet open: " + std::to_string(total * sizeof(pqr::PageRec)) + " B for the page table");
            }
            poison_device(d_recs, total * sizeof(pqr::PageRec), st);
            HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), nchunks * sizeof(pqr::ChunkDesc), hipMemcpyHostToDevice, st));
            pq_walk_kernel<true><<<grid, 64, 0, st>>>(h.d_bytes, d_chunks, nchunks, d_counts, d_recs, d_ctrl);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(recs.data(), d_recs, total * sizeof(pqr::PageRec), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&err, d_ctrl, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return OXH_OK;
        }();
        if (rc != OXH_OK) (void)hipStreamSynchronize(st);
        if (d_recs) (void)hipFree(d_recs);
        if (rc) return rc;
        if (err) {
            const uint64_t ch = std::min<uint64_t>(err, nchunks) - 1;  // the last chunk that failed
            return fail(OXH_ERR_INVALID, "parquet open: row group " + std::to_string(ch / ncols) + ", column '" + f.leaves[ch % ncols].name +
                                             "': a page header runs past its chunk, has negative sizes or unequal ones on a page that is not compressed, or the pages' values are not the chunk's num_values");
        }
        // a record names bytes of its own chunk only (the kernel checked; the table is what the column kernels trust)
        for (uint64_t k = 0; k < nchunks; ++k)
            for (uint32_t j = 0; j < counts[k]; ++j) {
                const pqr::PageRec& r = recs[chunks[k].page0 + j];
                if (r.body < chunks[k].at || r.body - chunks[k].at > chunks[k].bytes || r.file_size > chunks[k].bytes - (r.body - chunks[k].at) ||
                    r.body_size > pqr::kMaxPage || (!(r.flags & pqr::kPageInImage) && r.body_size != r.file_size))
                    return fail(OXH_ERR_HIP, "parquet open: a page record is not inside its chunk (did the buffer change during the call?)");
            }
        rc = inflate_pages(h, chunks, counts, recs, lease, st);
        if (rc) return rc;
    }
    uint64_t unreadable = 0;
    h.columns.resize(ncols);
    for (uint64_t c = 0; c < ncols; ++c) {
        if (f.leaves[c].cause.empty())
            h.columns[c] = (f.leaves[c].list ? pqr::list_pages : pqr::column_pages)(f, c, chunks, counts, recs);
        else
            h.columns[c].cause = f.leaves[c].cause;
        unreadable += !h.columns[c].cause.empty();
    }
    for (const pqr::PageRec& r : recs) (r.kind == (uint32_t)pqr::kPageDict ? h.dict_pages : h.data_pages) += 1;
    stats8[0] = f.nrows, stats8[1] = ncols, stats8[2] = f.group_rows.size(), stats8[3] = h.data_pages, stats8[4] = h.dict_pages;
    stats8[5] = f.footer_bytes, stats8[6] = unreadable, stats8[7] = h.pages_inflated;
    STEP("parquet open: %llu B, %llu rows x %llu columns, %llu pages", (unsigned long long)h.nbytes, (unsigned long long)f.nrows,
         (unsigned long long)ncols, (unsigned long long)recs.size());
    return OXH_OK;
}

struct Selection {
    uint32_t nsel;
    const uint32_t* col_idx;
    const uint32_t* types;
};

// Working memory of one selected column (offsets into a lease); the columns run one after the other in it.
struct ColumnLease {
    uint64_t ctrl, pages, dicts, words, prefix, page_valid, idx, cell_at, cell_len, dict_at, dict_len, lens, src, len_scan, sums, total;
    ColumnLease(uint64_t nrows, uint32_t nsel, uint64_t npages, uint64_t ndicts, uint64_t words_, uint64_t entries, bool strings, bool write) {
        csv::Carver carve;
        ctrl = carve((uint64_t)nsel * pqr::kColWords * 8);
        pages = carve(npages * sizeof(pqr::DataPage)), dicts = carve(ndicts * sizeof(pqr::DictPage));
        words = carve(words_ * 8), prefix = carve(words_ * 4), page_valid = carve(npages * 4), idx = carve(nrows * 4);
        cell_at = carve(strings ? nrows * 4 : 0), cell_len = carve(strings ? nrows * 4 : 0);
        dict_at = carve(strings ? entries * 4 : 0), dict_len = carve(strings ? entries * 4 : 0);
        lens = carve(strings && write ? nrows * 4 : 0), src = carve(strings && write ? nrows * 8 : 0), len_scan = carve(strings && write ? nrows * 8 : 0);
        sums = carve((csv::scan_tiles_of(nrows) + 1) * 8);
        total = carve.at;
    }
};

// Every selected column: measured, and with outputs written into the device buffers the tables name. ctrl: per
// selection its kColWords words on the host.
int columns_device(ParquetHandle& h, const Selection& s, bool write, void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity,
                   const uint64_t* capacity, std::vector<unsigned long long>& ctrl, hipStream_t st) {
    using namespace oxh;
    const uint64_t n = h.nrows();
    if (csv::scan_tiles_of(n) != scan_tiles(n)) return fail(OXH_ERR_HIP, "parquet: the scan's tile is not the lease's");
    uint64_t npages = 0, ndicts = 0, words = 0, entries = 0;
    bool strings = false;
    for (uint32_t k = 0; k < s.nsel; ++k) {
        const pqr::ColumnPages& cp = h.columns[s.col_idx[k]];
        npages = std::max<uint64_t>(npages, cp.data.size()), ndicts = std::max<uint64_t>(ndicts, cp.dicts.size());
        words = std::max(words, cp.words), entries = std::max(entries, cp.entries);
        strings |= csv::is_string(s.types[k]);
    }
    const ColumnLease at(n, s.nsel, npages, ndicts, words, entries, strings, write);
    ctrl.assign((size_t)s.nsel * pqr::kColWords, 0);
    ScratchLease lease(st);
    void* lbase = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet columns: " + std::to_string(at.total) + " B of page lists, validity words, indices, cells and their scan");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    const uint64_t ctrl_words = (uint64_t)s.nsel * pqr::kColWords;
    int rc = [&]() -> int {
        pq_clear_kernel<<<1, 256, 0, st>>>(d_ctrl, ctrl_words);
        HIP_TRY(hipGetLastError());
        for (uint32_t k = 0; k < s.nsel; ++k) {
            const uint32_t col = s.col_idx[k], type = s.types[k];
            const pqr::ColumnPages& cp = h.columns[col];
            const pqr::Leaf& leaf = h.footer.leaves[col];
            unsigned long long* c = d_ctrl + (size_t)k * pqr::kColWords;
            PqColumn v{h.d_bytes, h.image, (const pqr::DataPage*)(b + at.pages), (const pqr::DictPage*)(b + at.dicts), n, (uint32_t)cp.data.size(),
                       (uint32_t)cp.dicts.size(), leaf.required ? 0u : 1u, (uint64_t*)(b + at.words), (uint32_t*)(b + at.prefix),
                       (uint32_t*)(b + at.page_valid), (uint32_t*)(b + at.idx), (uint32_t*)(b + at.cell_at), (uint32_t*)(b + at.cell_len),
                       (uint32_t*)(b + at.dict_at), (uint32_t*)(b + at.dict_len)};
            // the lists are the handle's: they outlive the copies
            if (!cp.data.empty()) HIP_TRY(hipMemcpyAsync(b + at.pages, cp.data.data(), cp.data.size() * sizeof(pqr::DataPage), hipMemcpyHostToDevice, st));
            if (!cp.dicts.empty()) HIP_TRY(hipMemcpyAsync(b + at.dicts, cp.dicts.data(), cp.dicts.size() * sizeof(pqr::DictPage), hipMemcpyHostToDevice, st));
            const unsigned pgrid = wave_grid(v.npages), rgrid = row_grid(n);
            if (v.optional) {
                pq_levels_kernel<<<pgrid, 256, 0, st>>>(v, c);
                HIP_TRY(hipGetLastError());
            }
            const bool is_str = csv::is_string(type);
            if (cp.indices) {
                pq_index_kernel<<<pgrid, 256, 0, st>>>(v, c);
                HIP_TRY(hipGetLastError());
            }
            if (!is_str && !write) continue;  // the measure of a fixed column is its nulls and its coded values
            if (is_str) {
                pq_chase_kernel<false><<<pgrid, 256, 0, st>>>(v, c);
                HIP_TRY(hipGetLastError());
                if (v.ndicts) {
                    pq_chase_kernel<true><<<wave_grid(v.ndicts), 256, 0, st>>>(v, c);
                    HIP_TRY(hipGetLastError());
                }
                uint32_t* d_lens = write ? (uint32_t*)(b + at.lens) : nullptr;
                uint64_t* d_src = write ? (uint64_t*)(b + at.src) : nullptr;
                pq_strlen_kernel<<<rgrid, 256, 0, st>>>(v, d_lens, d_src, write ? d_validity[k] : nullptr, c);
                HIP_TRY(hipGetLastError());
                if (!write) continue;
                // the bytes are known before anything is copied: a column above its capacity writes nothing
                unsigned long long got[pqr::kColWords];
                HIP_TRY(hipMemcpyAsync(got, c, sizeof got, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (got[pqr::kColErr]) continue;  // reported below
                const std::string what = csv::string_bytes_error(type, got[pqr::kColBytes], true, capacity[k]);
                if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet columns: selection " + std::to_string(k) + ": " + what);
                uint64_t* d_scan = (uint64_t*)(b + at.len_scan);
                int r = exclusive_scan_u32(d_lens, n, d_scan, (unsigned long long*)(b + at.sums), st);
                if (r) return r;
                pq_strcopy_kernel<<<rgrid, 256, 0, st>>>(v, d_lens, d_src, d_scan, got[pqr::kColBytes], d_offsets[k], type == OXH_CSV_STRING64,
                                                         (uint8_t*)d_values[k], c);
            } else if (type == OXH_CSV_BOOL) {
                pq_bool_kernel<<<rgrid, 256, 0, st>>>(v, (uint8_t*)d_values[k], d_validity[k], c);
            } else if (leaf.physical == pqr::kInt64 || leaf.physical == pqr::kDouble) {
                pq_fixed_kernel<8, 8, false><<<rgrid, 256, 0, st>>>(v, d_values[k], d_validity[k], c);
            } else if (csv::is_narrow(type)) {
                pq_fixed_kernel<4, 4, false><<<rgrid, 256, 0, st>>>(v, d_values[k], d_validity[k], c);
            } else if (type == OXH_CSV_FLOAT64) {
                pq_fixed_kernel<4, 8, true><<<rgrid, 256, 0, st>>>(v, d_values[k], d_validity[k], c);
            } else {
                pq_fixed_kernel<4, 8, false><<<rgrid, 256, 0, st>>>(v, d_values[k], d_validity[k], c);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(ctrl.data(), d_ctrl, ctrl_words * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            const unsigned long long err = ctrl[(size_t)k * pqr::kColWords + pqr::kColErr];
            if (!err) continue;
            const std::string col = "column '" + h.footer.leaves[s.col_idx[k]].name + "': ";
            const char* what = err & pqr::kErrLevels   ? "a page's definition levels are malformed or end early"
                               : err & pqr::kErrIndex  ? "a page's index or boolean runs are malformed, end early, or name an entry beyond the dictionary"
                               : err & pqr::kErrChain  ? "a byte array's length leaves its page"
                               : err & pqr::kErrValues ? "a page is shorter than its values"
                                                       : "a string's place is outside its column's bytes (did the buffer change during the call?)";
            return fail(err & pqr::kErrPlace ? OXH_ERR_HIP : OXH_ERR_INVALID, "parquet columns: " + col + what);
        }
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

void fill_stats(const ParquetHandle& h, const Selection& s, const std::vector<unsigned long long>& ctrl, uint64_t* value_bytes, uint64_t* stats4) {
    for (uint32_t k = 0; k < s.nsel; ++k) {
        const unsigned long long* c = ctrl.data() + (size_t)k * pqr::kColWords;
        const pqr::ColumnPages& cp = h.columns[s.col_idx[k]];
        value_bytes[k] = csv::is_string(s.types[k]) ? c[pqr::kColBytes] : csv::fixed_value_bytes(s.types[k], h.nrows());
        stats4[4 * k] = c[pqr::kColNulls], stats4[4 * k + 1] = c[pqr::kColDictValues], stats4[4 * k + 2] = cp.data.size() + cp.dicts.size();
        stats4[4 * k + 3] = value_bytes[k];
    }
}

// What both forms of oxh_parquet_columns_* do first. `done`: nothing left to do.
int columns_enter(void* handle, const csv::ColumnsArgs& a, ParquetHandle*& h, bool& done) {
    done = false;
    h = handle_of(handle);
    if (!h) return fail(OXH_ERR_INVALID, "parquet columns: the handle is NULL or not a Parquet handle");
    csv::ColumnsArgs full = a;
    full.nrows = h->nrows(), full.ncols = h->ncols();
    const std::string what = csv::columns_error(full, OXH_CSV_FLOAT32);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet columns: " + what);
    for (uint32_t k = 0; k < a.nsel; ++k) {
        const pqr::Leaf& leaf = h->footer.leaves[a.col_idx[k]];
        const std::string col = "selection " + std::to_string(k) + ", column '" + leaf.name + "': ";
        if (!h->columns[a.col_idx[k]].cause.empty()) return fail(OXH_ERR_INVALID, "parquet columns: " + col + h->columns[a.col_idx[k]].cause);
        if (leaf.list) return fail(OXH_ERR_INVALID, "parquet columns: " + col + "a list column: oxh_parquet_lists_* read it");
        if (!pqr::type_fits(leaf.physical, a.types[k]))
            return fail(OXH_ERR_INVALID, "parquet columns: " + col + "physical type " + pqr::physical_name(leaf.physical) + " is not read as type " + std::to_string(a.types[k]));
    }
    if (a.nsel == 0 || h->nrows() == 0) {
        for (uint32_t k = 0; k < a.nsel; ++k) a.value_bytes[k] = 0;
        for (uint32_t k = 0; k < 4 * a.nsel; ++k) a.stats4[k] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(h->ctx);
}

int columns_run(ParquetHandle& h, const csv::ColumnsArgs& a, void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity,
                const uint64_t* capacity, hipStream_t st) {
    const Selection s{a.nsel, a.col_idx, a.types};
    std::vector<unsigned long long> ctrl;
    int rc = columns_device(h, s, d_values != nullptr, d_values, d_offsets, d_validity, capacity, ctrl, st);
    if (rc) return rc;
    if (!d_values)
        for (uint32_t k = 0; k < a.nsel; ++k) {
            if (!csv::is_string(a.types[k])) continue;
            const std::string what = csv::string_bytes_error(a.types[k], ctrl[(size_t)k * pqr::kColWords + pqr::kColBytes], false, 0);
            if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet columns: selection " + std::to_string(k) + ": " + what);
        }
    fill_stats(h, s, ctrl, a.value_bytes, a.stats4);
    return OXH_OK;
}

int open_args(const uint8_t* bytes, uint64_t nbytes, uint32_t flags, void* const* out, const uint64_t* stats8) {
    const std::string what = pqr::open_error(bytes, nbytes, flags, out, stats8);
    return what.empty() ? OXH_OK : fail(OXH_ERR_INVALID, "parquet open: " + what);
}

}  // namespace

extern "C" {

int oxh_parquet_open_device(oxh_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, uint32_t flags, void** out, uint64_t* stats8, void* stream) {
    int rc = open_args(d_bytes, nbytes, flags, out, stats8);
    if (rc) return rc;
    if ((rc = device_enter(ctx))) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::unique_ptr<ParquetHandle> h(new ParquetHandle);
    h->ctx = ctx, h->device = ctx->device, h->d_bytes = d_bytes, h->nbytes = nbytes;
    uint8_t ends[12] = {};
    if (nbytes >= 12) {
        HIP_TRY(hipMemcpyAsync(ends, d_bytes, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ends + 4, d_bytes + nbytes - 8, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    uint64_t at = 0, len = 0;
    const std::string what = pqr::footer_place(ends, ends + 4, nbytes, at, len);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet open: " + what);
    std::vector<uint8_t> meta;
    try {
        meta.resize(len);
    } catch (const std::bad_alloc&) {
        return fail(OXH_ERR_NOMEM, "parquet open: " + std::to_string(len) + " B for the footer on the host");
    }
    if (len) {
        HIP_TRY(hipMemcpyAsync(meta.data(), d_bytes + at, len, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    pqr::Footer f = pqr::read_footer(meta.data(), len, at, nbytes, flags & OXH_PARQUET_INFLATE, flags & OXH_PARQUET_INFLATE_ZSTD);
    if (!f.error.empty()) return fail(OXH_ERR_INVALID, "parquet open: " + f.error);
    take_footer(*h, std::move(f));
    uint64_t stats[8] = {};
    rc = open_run(*h, stats, st);
    if (rc) return rc;
    memcpy(stats8, stats, sizeof stats);
    *out = h.release();
    return OXH_OK;
}

int oxh_parquet_open_host(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint32_t flags, void** out, uint64_t* stats8) {
    int rc = open_args(bytes, nbytes, flags, out, stats8);
    if (rc) return rc;
    uint64_t at = 0, len = 0;
    const uint8_t none[8] = {};
    const std::string what = pqr::footer_place(nbytes >= 12 ? bytes : none, nbytes >= 12 ? bytes + nbytes - 8 : none, nbytes, at, len);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet open: " + what);
    pqr::Footer f = pqr::read_footer(bytes + at, len, at, nbytes, flags & OXH_PARQUET_INFLATE, flags & OXH_PARQUET_INFLATE_ZSTD);
    if (!f.error.empty()) return fail(OXH_ERR_INVALID, "parquet open: " + f.error);
    if ((rc = device_enter(ctx))) return rc;
    hipStream_t st = ctx->stream;
    std::unique_ptr<ParquetHandle> h(new ParquetHandle);
    h->ctx = ctx, h->device = ctx->device, h->nbytes = nbytes;
    take_footer(*h, std::move(f));
    if (hipMalloc(&h->owned, nbytes) != hipSuccess) {
        (void)hipGetLastError();
        h->owned = nullptr;
        return fail(OXH_ERR_NOMEM, "parquet open: " + std::to_string(nbytes) + " B for the file on the device");
    }
    oxh::poison_device(h->owned, nbytes, st);
    h->d_bytes = h->owned;
    HIP_TRY(hipMemcpyAsync(h->owned, bytes, nbytes, hipMemcpyHostToDevice, st));
    uint64_t stats[8] = {};
    rc = open_run(*h, stats, st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // a file without a chunk launched nothing: the copy up is done before the caller's bytes go
    memcpy(stats8, stats, sizeof stats);
    *out = h.release();
    return OXH_OK;
}

int oxh_parquet_close(void* parquet) {
    if (!parquet) return OXH_OK;
    ParquetHandle* h = handle_of(parquet);
    if (!h) return fail(OXH_ERR_INVALID, "parquet close: not a Parquet handle");
    if (h->owned || h->image) (void)hipSetDevice(h->device);
    delete h;
    return OXH_OK;
}

int oxh_parquet_names(void* parquet, uint8_t* names, uint64_t capacity, uint64_t* name_offsets, uint64_t* names_bytes) {
    ParquetHandle* h = handle_of(parquet);
    if (!h) return fail(OXH_ERR_INVALID, "parquet names: the handle is NULL or not a Parquet handle");
    if (!name_offsets || !names_bytes) return fail(OXH_ERR_INVALID, "parquet names: name_offsets or names_bytes is NULL");
    *names_bytes = h->names.size();
    if (!names || capacity < h->names.size()) return OXH_OK;
    if (!h->names.empty()) memcpy(names, h->names.data(), h->names.size());
    for (uint64_t c = 0; c <= h->ncols(); ++c) name_offsets[c] = h->name_offsets[c];
    return OXH_OK;
}

int oxh_parquet_types(void* parquet, uint32_t* types4) {
    ParquetHandle* h = handle_of(parquet);
    if (!h) return fail(OXH_ERR_INVALID, "parquet types: the handle is NULL or not a Parquet handle");
    if (h->ncols() && !types4) return fail(OXH_ERR_INVALID, "parquet types: types4 is NULL");
    for (uint64_t c = 0; c < h->ncols(); ++c) {
        const pqr::Leaf& leaf = h->footer.leaves[c];
        types4[4 * c] = pqr::native_type(leaf.physical) | (leaf.list && pqr::list_element_read(leaf.physical) ? OXH_PARQUET_LIST : 0u);
        types4[4 * c + 1] = (uint32_t)leaf.physical, types4[4 * c + 2] = leaf.required;
        types4[4 * c + 3] = h->columns[c].cause.empty();
    }
    return OXH_OK;
}

int oxh_parquet_columns_device(void* parquet, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                               void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity, uint64_t* value_bytes, uint64_t* stats4,
                               void* stream) {
    const csv::ColumnsArgs a{0, 0, nsel, col_idx, types, value_capacity, d_values, d_offsets, d_validity, value_bytes, stats4};
    ParquetHandle* h = nullptr;
    bool done = false;
    int rc = columns_enter(parquet, a, h, done);
    if (rc || done) return rc;
    return columns_run(*h, a, d_values, d_offsets, d_validity, value_capacity, (hipStream_t)stream);
}

int oxh_parquet_columns_host(void* parquet, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                             void* const* values, void* const* offsets, uint8_t* const* validity, uint64_t* value_bytes, uint64_t* stats4) {
    const csv::ColumnsArgs a{0, 0, nsel, col_idx, types, value_capacity, values, offsets, validity, value_bytes, stats4};
    ParquetHandle* h = nullptr;
    bool done = false;
    int rc = columns_enter(parquet, a, h, done);
    if (rc || done) return rc;
    hipStream_t st = h->ctx->stream;
    if (!values) return columns_run(*h, a, nullptr, nullptr, nullptr, nullptr, st);
    // the device block holds what the caller's buffers hold: a string column its value_capacity
    const uint64_t n = h->nrows(), bitmap = (n + 7) / 8;
    std::vector<uint64_t> bytes(nsel), offset_bytes(nsel, 0), at_values(nsel), at_offsets(nsel), at_validity(nsel);
    uint64_t total = 0;
    auto carve = [&](uint64_t b) {
        const uint64_t here = total;
        total += (b + 15) & ~15ull;
        return here;
    };
    for (uint32_t k = 0; k < nsel; ++k) {
        const bool str = csv::is_string(types[k]);
        bytes[k] = str ? value_capacity[k] : csv::fixed_value_bytes(types[k], n);
        if (str) offset_bytes[k] = (n + 1) * (types[k] == OXH_CSV_STRING64 ? 8 : 4);
        at_values[k] = carve(bytes[k]), at_offsets[k] = carve(offset_bytes[k]), at_validity[k] = carve(bitmap);
    }
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet columns: " + std::to_string(total) + " B for the columns on the device");
    }
    oxh::poison_device(d_block, total + 16, st);
    std::vector<void*> d_values(nsel), d_offsets(nsel);
    std::vector<uint8_t*> d_validity(nsel);
    for (uint32_t k = 0; k < nsel; ++k)
        d_values[k] = d_block + at_values[k], d_offsets[k] = d_block + at_offsets[k], d_validity[k] = d_block + at_validity[k];
    rc = [&]() -> int {
        int r = columns_run(*h, a, d_values.data(), d_offsets.data(), d_validity.data(), value_capacity, st);
        if (r) return r;
        // the caller's arrays stay untouched unless everything succeeded
        for (uint32_t k = 0; k < nsel; ++k) {
            if (value_bytes[k]) HIP_TRY(hipMemcpyAsync(values[k], d_values[k], value_bytes[k], hipMemcpyDeviceToHost, st));
            if (offset_bytes[k]) HIP_TRY(hipMemcpyAsync(offsets[k], d_offsets[k], offset_bytes[k], hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(validity[k], d_validity[k], bitmap, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_block);
    return rc;
}

}  // extern "C"
