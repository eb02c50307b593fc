// oxen_amd/csrc/csv_read.hip -- CSV bytes in HBM to a record index and to typed Arrow columns (oxh_csv_*): what
// `oxen df data.csv` does first (core/df/tabular.rs:39-71 read_df_csv). The rules are stated in
// include/oxen_hash.h "CSV" (DESIGN.md §4 "CSV"); a cell's text as a value is csv_number.hpp's, the code
// tests/native/csv_host_test.cpp runs on the host; the checks, the sizes and the deferred floats are csv_host.hpp's.
//
// The index (oxh_csv_open_*), on one stream:
//   classify  csv_classify_kernel: a lane loads 16 bytes of the 16-byte aligned space around d_bytes (one
//             global_load_dwordx4; bytewise at the head and the tail, so any alignment works), builds its 16-bit
//             masks of quote, separator and '\n'; a workgroup tile (256 lanes, 4 KiB) writes its quote count;
//   scan      exclusive_scan_u32 over the tiles' quote counts: a tile starts inside quotes iff its sum is odd;
//   count     csv_delims_kernel<false>: the masks again; the quote parity in front of every byte by an in-lane
//             prefix-xor (shifts), across lanes by the parity of popcll(ballot & lanes below), across waves
//             through LDS; per tile the delimiters outside quotes and how many of them end a record. The position
//             one past the last byte ends the last record unless the last byte did;
//   scan x 2, then csv_delims_kernel<true>: ends[] = the position of every delimiter outside quotes, ascending;
//             rec_end[] = for every record the place of its end in ends[];
//   row map   csv_keep_kernel (a mask word and a count per 64 records: not empty), the scan, csv_rowmap_kernel:
//             row_rec[] = the kept records; csv_shape_kernel: ncols from the first kept record, the short and
//             long records.
// The columns (oxh_csv_columns_*), one lane per row, 64 rows per wave: csv_fixed_kernel parses INT64 / FLOAT64 /
// BOOL cells and builds the validity word, the bool word and the deferred word by __ballot; csv_str_len_kernel,
// the scan and csv_str_copy_kernel write a string column (cells of kLongCell bytes and more by a whole wave).
// Deferred floats: the scan over the per-block counts, csv_defer_emit_kernel, the host conversion,
// csv_defer_scatter_kernel. No workgroup ever waits for another; launches order the steps. A place from a scan is
// checked before it is stored through: a bad one sets the error word (OXH_ERR_HIP).
#include "capi_internal.hpp"
#include "columns.hpp"
#include "csv_host.hpp"

using namespace oxh::capi;

namespace oxh {

__constant__ double kCsvPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

constexpr uint32_t kCsvTileBytes = csv::kTileBytes;
constexpr uint32_t kCsvLongCell = csv::kLongCell;
constexpr uint32_t kCsvDeferSlot = csv::kDeferSlot;
constexpr unsigned long long kCsvErrPlace = 4;
// ctrl words of an open: the error word, "ended inside quotes", the short and long records, ncols, and the
// header record (its first field's place in ends[], its first byte)
constexpr int kCsvCtrlErr = 0, kCsvCtrlInside = 1, kCsvCtrlShort = 2, kCsvCtrlLong = 3, kCsvCtrlNcols = 4, kCsvCtrlHdrFirst = 5,
              kCsvCtrlHdrStart = 6, kCsvCtrlWords = 8;
// ctrl words of one selected column: stats4's first three, the string bytes, the error word
constexpr int kColEmpty = 0, kColBad = 1, kColDeferred = 2, kColBytes = 3, kColErr = 4, kColWords = 8;

// What the column kernels read of a handle.
struct CsvView {
    const uint8_t* bytes;
    const uint32_t* ends;
    const uint32_t* rec_end;
    const uint32_t* row_rec;
    uint64_t nrows;
    uint32_t hdr;    // 1: row_rec[0] is the header
    uint32_t quote;  // kNoQuote: none
};

struct CsvCell {
    uint32_t start, len;  // the field value, quotes off (doubled quotes inside still doubled)
    bool present, quoted;
};

// The first field's place in ends[] and the field count of record r.
__device__ __forceinline__ void csv_record(const uint32_t* rec_end, uint32_t r, uint32_t& first, uint32_t& nfields) {
    first = r ? rec_end[r - 1] + 1 : 0;
    nfields = rec_end[r] - first + 1;
}

__device__ __forceinline__ CsvCell csv_cell(const CsvView& v, uint64_t row, uint32_t col) {
    CsvCell c{0, 0, false, false};
    uint32_t first, nfields;
    csv_record(v.rec_end, v.row_rec[row + v.hdr], first, nfields);
    if (col >= nfields) return c;
    const uint32_t e = first + col;
    uint32_t start = e ? v.ends[e - 1] + 1 : 0, end = v.ends[e];
    if (col + 1 == nfields && end > start && v.bytes[end - 1] == '\r') --end;  // the record's own last field
    const uint8_t* p = v.bytes + start;
    uint32_t len = end - start;
    c.quoted = csvnum::strip_quotes(p, len, v.quote);
    c.start = (uint32_t)(p - v.bytes), c.len = len, c.present = true;
    return c;
}

// ---------------------------------------------------------------- the index
__device__ __forceinline__ void csv_word_masks(uint32_t w, uint32_t at, uint32_t sep, uint32_t quote, uint32_t& q, uint32_t& s, uint32_t& nl) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = (w >> (8 * k)) & 0xFF;
        q |= (uint32_t)(c == quote) << (at + k);
        s |= (uint32_t)(c == sep) << (at + k);
        nl |= (uint32_t)(c == '\n') << (at + k);
    }
}

// The lane's 16 bytes at v0 (a multiple of 16) of the aligned space; the buffer is [lo, hi) of it. A byte outside
// the buffer is in no mask and is never loaded.
__device__ __forceinline__ void csv_lane_masks(const uint8_t* base, uint64_t v0, uint64_t lo, uint64_t hi, uint32_t sep, uint32_t quote,
                                               uint32_t& q, uint32_t& s, uint32_t& nl) {
    q = s = nl = 0;
    if (v0 >= lo && v0 + 16 <= hi) {
        const uint4 w = *(const uint4*)(base + v0);
        csv_word_masks(w.x, 0, sep, quote, q, s, nl);
        csv_word_masks(w.y, 4, sep, quote, q, s, nl);
        csv_word_masks(w.z, 8, sep, quote, q, s, nl);
        csv_word_masks(w.w, 12, sep, quote, q, s, nl);
    } else if (v0 + 16 > lo && v0 < hi) {
        for (uint32_t j = 0; j < 16; ++j) {
            const uint64_t at = v0 + j;
            if (at < lo || at >= hi) continue;
            const uint32_t c = base[at];
            q |= (uint32_t)(c == quote) << j, s |= (uint32_t)(c == sep) << j, nl |= (uint32_t)(c == '\n') << j;
        }
    }
}

__global__ __launch_bounds__(256) void csv_classify_kernel(const uint8_t* __restrict__ base, uint64_t lo, uint64_t hi, uint32_t sep,
                                                           uint32_t quote, uint64_t ntiles, uint32_t* __restrict__ tile_quotes) {
    __shared__ uint32_t part[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // uniform in the workgroup
        uint32_t q, s, nl;
        csv_lane_masks(base, t * kCsvTileBytes + 16ull * threadIdx.x, lo, hi, sep, quote, q, s, nl);
        uint32_t cnt = __popc(q);
#pragma unroll
        for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        __syncthreads();  // the words of the tile before have been read
        if (lane == 0) part[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) tile_quotes[t] = part[0] + part[1] + part[2] + part[3];
    }
}

// EMIT false: tile_delims[t] / tile_recs[t] = the tile's delimiters outside quotes / those that end a record.
// EMIT true (the two are scanned): ends[] and rec_end[].
template <bool EMIT>
__global__ __launch_bounds__(256) void csv_delims_kernel(const uint8_t* __restrict__ base, uint64_t lo, uint64_t hi, uint32_t sep, uint32_t quote,
                                                         uint64_t ntiles, const uint64_t* __restrict__ quote_scan,
                                                         uint32_t* __restrict__ tile_delims, uint32_t* __restrict__ tile_recs,
                                                         const uint64_t* __restrict__ delim_scan, const uint64_t* __restrict__ rec_scan,
                                                         uint32_t* __restrict__ ends, uint32_t* __restrict__ rec_end, uint64_t nends,
                                                         uint64_t nrec, unsigned long long* __restrict__ ctrl) {
    __shared__ uint32_t wave_parity[4], wave_sum[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    unsigned long long bad = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // uniform in the workgroup
        const uint64_t v0 = t * kCsvTileBytes + 16ull * threadIdx.x;
        uint32_t q, s, nl;
        csv_lane_masks(base, v0, lo, hi, sep, quote, q, s, nl);
        // bit j of px: the parity of the lane's quotes at bytes 0 .. j
        uint32_t px = q;
        px ^= px << 1, px ^= px << 2, px ^= px << 4, px ^= px << 8;
        const unsigned long long odd = __ballot(__popc(q) & 1);
        __syncthreads();  // the words of the tile before have been read
        if (lane == 0) wave_parity[wave] = __popcll(odd) & 1;
        __syncthreads();
        uint32_t entry = (uint32_t)(quote_scan[t] & 1);
        for (unsigned w = 0; w < wave; ++w) entry ^= wave_parity[w];
        const uint32_t carry = entry ^ (__popcll(odd & below) & 1);
        // bit j: byte j lies inside quotes (for a byte that is no quote: the quotes in front of it are odd)
        const uint32_t inside = (carry ? ~px : px) & 0xFFFF;
        uint32_t delim = (s | nl) & ~inside, rec = nl & ~inside;
        if (hi >= v0 && hi < v0 + 16) {  // one past the last byte: ends the last record unless the last byte did
            const uint32_t j = (uint32_t)(hi - v0);
            const uint32_t inside_end = (inside >> j) & 1;
            const bool last_nl = j ? (nl >> (j - 1)) & 1 : base[hi - 1] == '\n';
            if (!(last_nl && !inside_end)) delim |= 1u << j, rec |= 1u << j;
            if (!EMIT) ctrl[kCsvCtrlInside] = inside_end;
        }
        // both counts in one word: a tile has at most 4 097 of either
        const uint32_t mine = __popc(delim) | (__popc(rec) << 16);
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if (lane >= (unsigned)off) incl += up;
        }
        __syncthreads();
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = incl - mine;
        for (unsigned w = 0; w < wave; ++w) before += wave_sum[w];
        if (!EMIT) {
            if (threadIdx.x == 255) {
                const uint32_t total = before + mine;
                tile_delims[t] = total & 0xFFFF, tile_recs[t] = total >> 16;
            }
        } else {
            uint64_t pd = delim_scan[t] + (before & 0xFFFF), pr = rec_scan[t] + (before >> 16);
            while (delim) {
                const uint32_t j = __builtin_ctz(delim);
                delim &= delim - 1;
                if (pd < nends)
                    ends[pd] = (uint32_t)(v0 + j - lo);
                else
                    bad |= kCsvErrPlace;
                if ((rec >> j) & 1) {
                    if (pr < nrec)
                        rec_end[pr] = (uint32_t)pd;
                    else
                        bad |= kCsvErrPlace;
                    ++pr;
                }
                ++pd;
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kCsvCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// mask[k] = the kept records (not empty) of block k (records 64k .. 64k + 63), counts[k] = how many.
__global__ __launch_bounds__(256) void csv_keep_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ ends,
                                                       const uint32_t* __restrict__ rec_end, uint64_t nrec, uint64_t* __restrict__ mask,
                                                       uint32_t* __restrict__ counts) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (nrec + stride - 1) / stride;  // uniform: every lane reaches the ballot
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t r = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool kept = false;
        if (r < nrec) {
            uint32_t first, nfields;
            csv_record(rec_end, (uint32_t)r, first, nfields);
            const uint32_t start = first ? ends[first - 1] + 1 : 0, len = ends[first] - start;
            kept = !(nfields == 1 && (len == 0 || (len == 1 && bytes[start] == '\r')));
        }
        const unsigned long long word = __ballot(kept);
        if (lane == 0 && r < nrec) mask[r >> 6] = word, counts[r >> 6] = (uint32_t)__popcll(word);
    }
}

__global__ __launch_bounds__(256) void csv_rowmap_kernel(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ bases, uint64_t nrec,
                                                         uint32_t* __restrict__ row_rec, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += stride) {
        const uint64_t word = mask[r >> 6];
        if (!((word >> lane) & 1)) continue;
        const uint64_t place = bases[r >> 6] + (uint64_t)__popcll(word & ((1ull << lane) - 1));
        if (place <= r)  // the kept records before record r: never a store outside the nrec places
            row_rec[place] = (uint32_t)r;
        else
            bad |= kCsvErrPlace;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kCsvCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (row_rec is written, *nkept has landed) ncols and the header record into ctrl; the short and long data records.
__global__ __launch_bounds__(256) void csv_shape_kernel(const uint32_t* __restrict__ ends, const uint32_t* __restrict__ rec_end,
                                                        const uint32_t* __restrict__ row_rec, const unsigned long long* __restrict__ nkept,
                                                        uint32_t hdr, unsigned long long* __restrict__ ctrl) {
    const uint64_t kept = *nkept;
    if (!kept) return;
    uint32_t first, ncols;
    csv_record(rec_end, row_rec[0], first, ncols);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctrl[kCsvCtrlNcols] = ncols, ctrl[kCsvCtrlHdrFirst] = first;
        ctrl[kCsvCtrlHdrStart] = first ? ends[first - 1] + 1 : 0;
    }
    unsigned long long few = 0, many = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = hdr + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < kept; k += stride) {
        uint32_t f, nfields;
        csv_record(rec_end, row_rec[k], f, nfields);
        few += nfields < ncols, many += nfields > ncols;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        few += (unsigned long long)__shfl_xor((long long)few, off, 64);
        many += (unsigned long long)__shfl_xor((long long)many, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (few) atomicAdd(&ctrl[kCsvCtrlShort], few);
        if (many) atomicAdd(&ctrl[kCsvCtrlLong], many);
    }
}

// ---------------------------------------------------------------- the columns
// A wave's word of 64 rows as the up to 8 bytes of an Arrow bitmap from bit 0 that lie within the n rows:
// row0 = the wave's first row (a multiple of 64).
__device__ __forceinline__ void csv_store_word(uint8_t* bitmap, unsigned long long word, uint64_t row0, uint64_t n, unsigned lane) {
    if (bitmap && lane < 8 && row0 + 8 * lane < n) bitmap[(row0 >> 3) + lane] = (uint8_t)(word >> (8 * lane));
}

// INT64 / FLOAT64 (values: 8 bytes per row) and BOOL (values: a bit per row). With NULL outputs: the counts only.
template <uint32_t TYPE>
__global__ __launch_bounds__(256) void csv_fixed_kernel(const CsvView v, uint32_t col, uint64_t* __restrict__ values, uint8_t* __restrict__ bits,
                                                        uint8_t* __restrict__ validity, uint64_t* __restrict__ defer_mask,
                                                        uint32_t* __restrict__ defer_counts, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = v.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    unsigned long long n_empty = 0, n_bad = 0, n_deferred = 0;  // the same in every lane of a wave
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool valid = false, empty = false, deferred = false, truth = false;
        uint64_t word = 0;
        if (i < n) {
            const CsvCell c = csv_cell(v, i, col);
            if (!c.present || c.len == 0) {
                empty = true;
            } else {
                const uint8_t* p = v.bytes + c.start;
                if (TYPE == OXH_CSV_INT64) {
                    int64_t x = 0;
                    valid = csvnum::parse_int64(p, c.len, x) == csvnum::kIntValue;
                    word = valid ? (uint64_t)x : 0;
                } else if (TYPE == OXH_CSV_FLOAT64) {
                    uint64_t m;
                    int32_t e10;
                    bool neg;
                    const uint32_t kind = csvnum::parse_float(p, c.len, m, e10, neg);
                    valid = kind != csvnum::kFloatNoMatch;
                    deferred = kind == csvnum::kFloatDeferred;
                    if (kind == csvnum::kFloatExact)
                        word = (uint64_t)__double_as_longlong(csvnum::exact_value(m, e10, neg, kCsvPow10));
                    else if (kind == csvnum::kFloatInf)
                        word = csvnum::kInfBits | (neg ? csvnum::kSignBit : 0);
                    else if (kind == csvnum::kFloatNan)
                        word = csvnum::kQuietNan | (neg ? csvnum::kSignBit : 0);
                } else {
                    valid = csvnum::parse_bool(p, c.len, truth);
                    truth = truth && valid;
                }
            }
            if (TYPE != OXH_CSV_BOOL && values) values[i] = word;
        }
        const uint64_t row0 = i - lane;
        const unsigned long long vword = __ballot(valid);
        csv_store_word(validity, vword, row0, n, lane);
        if (TYPE == OXH_CSV_BOOL) csv_store_word(bits, __ballot(truth), row0, n, lane);
        n_empty += __popcll(__ballot(empty));
        n_bad += __popcll(__ballot(i < n && !valid && !empty));
        if (TYPE == OXH_CSV_FLOAT64) {
            const unsigned long long dword = __ballot(deferred);
            n_deferred += __popcll(dword);
            if (defer_mask && lane == 0 && i < n) defer_mask[i >> 6] = dword, defer_counts[i >> 6] = (uint32_t)__popcll(dword);
        }
    }
    if (lane == 0) {
        if (n_empty) atomicAdd(&ctrl[kColEmpty], n_empty);
        if (n_bad) atomicAdd(&ctrl[kColBad], n_bad);
        if (n_deferred) atomicAdd(&ctrl[kColDeferred], n_deferred);
    }
}

// (the masks are written, the counts scanned) For deferred cell number `place` of the column: list[3 place ..] =
// {row, where its text starts, its length}, and the first kCsvDeferSlot bytes of the text in its slot.
__global__ __launch_bounds__(256) void csv_defer_emit_kernel(const CsvView v, uint32_t col, const uint64_t* __restrict__ mask,
                                                             const uint64_t* __restrict__ bases, uint64_t ndeferred, uint32_t* __restrict__ list,
                                                             uint8_t* __restrict__ slots, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < v.nrows; i += stride) {
        const uint64_t word = mask[i >> 6];
        if (!((word >> lane) & 1)) continue;
        const uint64_t place = bases[i >> 6] + (uint64_t)__popcll(word & ((1ull << lane) - 1));
        if (place >= ndeferred) {
            bad |= kCsvErrPlace;
            continue;
        }
        const CsvCell c = csv_cell(v, i, col);
        list[3 * place] = (uint32_t)i, list[3 * place + 1] = c.start, list[3 * place + 2] = c.len;
        const uint32_t take = c.len < kCsvDeferSlot ? c.len : kCsvDeferSlot;
        for (uint32_t k = 0; k < take; ++k) slots[place * kCsvDeferSlot + k] = v.bytes[c.start + k];
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The deferred texts longer than a slot, one wave each: jobs[2 k] = where text k starts in the buffer | its length
// << 32, jobs[2 k + 1] = its place in `text` (the host checked both against the buffer and summed the lengths).
__global__ __launch_bounds__(256) void csv_defer_long_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ jobs, uint64_t njobs,
                                                             uint8_t* __restrict__ text) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < njobs; k += stride)  // uniform in the wave
        copy_span_wave(text + jobs[2 * k + 1], bytes + (uint32_t)jobs[2 * k], jobs[2 * k] >> 32, lane);
}

__global__ __launch_bounds__(256) void csv_defer_scatter_kernel(const uint32_t* __restrict__ list, const uint64_t* __restrict__ converted,
                                                                uint64_t ndeferred, uint64_t nrows, uint64_t* __restrict__ values) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ndeferred; k += stride) {
        const uint32_t row = list[3 * k];
        if (row < nrows) values[row] = converted[k];
    }
}

// The n bytes at src with every doubled quote as one, by a whole wave (every lane calls it with the same
// arguments): 64 bytes a step; a quote at an odd place of its run of quotes is dropped, and a run may cross a
// step. Returns how many were dropped; COPY: the others go to dst in order.
template <bool COPY>
__device__ __forceinline__ uint32_t csv_wave_unescape(const uint8_t* src, uint32_t n, uint32_t quote, unsigned lane, uint8_t* dst) {
    const unsigned long long below = (1ull << lane) - 1;
    uint32_t dropped = 0, out = 0, run = 0;  // run: the parity of the run of quotes that ends with the step before
    for (uint32_t at = 0; at < n; at += 64) {
        const bool in = at + lane < n;
        const uint32_t c = in ? src[at + lane] : 0;
        const bool is_quote = in && c == quote;
        const unsigned long long m = __ballot(is_quote);
        const unsigned long long gaps = ~m & below;  // the lanes below that hold no quote
        const uint32_t place = gaps ? lane - (64 - (uint32_t)__builtin_clzll(gaps)) : lane + run;
        const bool drop = is_quote && (place & 1);
        const unsigned long long keep = __ballot(in && !drop);
        if (COPY && in && !drop) dst[out + __popcll(keep & below)] = (uint8_t)c;
        out += __popcll(keep);
        dropped += __popcll(__ballot(drop));
        run = __shfl(is_quote ? (place + 1) & 1 : 0u, 63, 64);
    }
    return dropped;
}

// lens[i] (may be NULL) = the bytes of row i's string; validity (may be NULL); ctrl: the nulls and the bytes.
__global__ __launch_bounds__(256) void csv_str_len_kernel(const CsvView v, uint32_t col, uint32_t* __restrict__ lens, uint8_t* __restrict__ validity,
                                                          unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = v.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    unsigned long long n_empty = 0, bytes = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        CsvCell c{0, 0, false, false};
        if (i < n) c = csv_cell(v, i, col);
        const bool valid = c.present && (c.len || c.quoted);
        uint32_t dropped = 0;
        const bool is_long = c.quoted && c.len >= kCsvLongCell;
        if (c.quoted && !is_long) {
            const uint8_t* p = v.bytes + c.start;
            for (uint32_t k = 0; k + 1 < c.len; ++k)
                if (p[k] == v.quote && p[k + 1] == v.quote) ++dropped, ++k;
        }
        unsigned long long todo = __ballot(is_long);
        while (todo) {  // uniform in the wave
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t d = csv_wave_unescape<false>(v.bytes + __shfl(c.start, src, 64), __shfl(c.len, src, 64), v.quote, lane, nullptr);
            if ((int)lane == src) dropped = d;
        }
        const uint32_t len = c.len - dropped;
        if (lens && i < n) lens[i] = len;
        csv_store_word(validity, __ballot(valid), i - lane, n, lane);
        n_empty += __popcll(__ballot(i < n && !valid));
        unsigned long long sum = len;
#pragma unroll
        for (int off = 32; off; off >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, off, 64);
        bytes += sum;
    }
    if (lane == 0) {
        if (n_empty) atomicAdd(&ctrl[kColEmpty], n_empty);
        if (bytes) atomicAdd(&ctrl[kColBytes], bytes);
    }
}

// (lens are written and scanned into starts) offsets[0 .. n] and the bytes of every string.
__global__ __launch_bounds__(256) void csv_str_copy_kernel(const CsvView v, uint32_t col, const uint32_t* __restrict__ lens,
                                                           const uint64_t* __restrict__ starts, uint64_t total, void* __restrict__ offsets,
                                                           uint32_t wide, uint8_t* __restrict__ values, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = v.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: the long cells are a whole wave's
    unsigned long long bad = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        CsvCell c{0, 0, false, false};
        uint64_t at = 0;
        uint32_t len = 0;
        if (i < n) {
            c = csv_cell(v, i, col);
            at = starts[i], len = lens[i];
            if (at + len > total || len > c.len) bad |= kCsvErrPlace, len = 0, c.len = 0;  // never a store outside the total bytes
            if (wide) {
                ((uint64_t*)offsets)[i] = at;
                if (i + 1 == n) ((uint64_t*)offsets)[n] = total;
            } else {
                ((uint32_t*)offsets)[i] = (uint32_t)at;
                if (i + 1 == n) ((uint32_t*)offsets)[n] = (uint32_t)total;
            }
        }
        const bool is_long = c.len >= kCsvLongCell;
        if (len && !is_long) {
            const uint8_t* p = v.bytes + c.start;
            uint8_t* d = values + at;
            if (len == c.len) {
                copy_span_lane(d, p, len);
            } else {
                uint32_t o = 0;
                for (uint32_t k = 0; k < c.len && o < len; ++k) {
                    d[o++] = p[k];
                    if (p[k] == v.quote && k + 1 < c.len && p[k + 1] == v.quote) ++k;
                }
            }
        }
        unsigned long long todo = __ballot(is_long && len);
        while (todo) {  // uniform in the wave
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint8_t* p = v.bytes + __shfl(c.start, src, 64);
            const uint32_t raw = __shfl(c.len, src, 64), out = __shfl(len, src, 64);
            uint8_t* d = values + (uint64_t)__shfl((long long)at, src, 64);
            if (raw == out)
                copy_span_wave(d, p, raw, lane);
            else
                (void)csv_wave_unescape<true>(p, raw, v.quote, lane, d);
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// bits[c] &= the class bits of every cell of column c among the first `rows` rows (bits start as all ones);
// some[c] |= 1 where a cell is not empty.
__global__ __launch_bounds__(256) void csv_infer_kernel(const CsvView v, uint64_t rows, uint32_t ncols, uint32_t* __restrict__ bits,
                                                        uint32_t* __restrict__ some) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (rows + stride - 1) / stride;  // uniform: every lane reaches the ballots
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        for (uint32_t c = 0; c < ncols; ++c) {
            uint32_t mine = csvnum::kAllOk;
            bool filled = false;
            if (i < rows) {
                const CsvCell cell = csv_cell(v, i, c);
                if (cell.present && cell.len) mine = csvnum::class_bits(v.bytes + cell.start, cell.len), filled = true;
            }
            const uint32_t all = (__ballot(mine & csvnum::kIntOk) == ~0ull ? csvnum::kIntOk : 0) |
                                 (__ballot(mine & csvnum::kFloatOk) == ~0ull ? csvnum::kFloatOk : 0) |
                                 (__ballot(mine & csvnum::kBoolOk) == ~0ull ? csvnum::kBoolOk : 0);
            const bool any = __ballot(filled) != 0;
            if (lane == 0) {
                if (all != csvnum::kAllOk) atomicAnd(&bits[c], all);
                if (any) atomicOr(&some[c], 1u);
            }
        }
    }
}

}  // namespace oxh

namespace {

namespace csv = oxh::csv;
using oxh::CsvView;

constexpr uint64_t kCsvMagic = 0x4F58484353563031ull;  // "OXHCSV01"

struct CsvHandle {
    uint64_t magic = kCsvMagic;
    oxh_ctx* ctx = nullptr;
    int device = 0;
    const uint8_t* d_bytes = nullptr;
    uint8_t* owned = nullptr;   // the host form's device copy
    uint64_t nbytes = 0;
    uint32_t sep = 0, quote = 0, flags = 0;
    uint32_t* block = nullptr;  // ends | rec_end | row_rec
    uint32_t *ends = nullptr, *rec_end = nullptr, *row_rec = nullptr;
    uint64_t nends = 0, nrec = 0, nkept = 0, nrows = 0, ncols = 0;
    std::vector<uint8_t> names;
    std::vector<uint64_t> name_offsets;
    ~CsvHandle() {
        magic = 0;
        if (block) (void)hipFree(block);
        if (owned) (void)hipFree(owned);
    }
    uint32_t hdr() const { return (flags & OXH_CSV_HAS_HEADER) && nkept ? 1 : 0; }
    CsvView view() const { return CsvView{d_bytes, ends, rec_end, row_rec, nrows, hdr(), quote}; }
};

unsigned cap_grid(uint64_t groups) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(groups, 1), 2048); }
unsigned row_grid(uint64_t n) { return cap_grid((n + 255) / 256); }

CsvHandle* handle_of(void* csv) {
    CsvHandle* h = (CsvHandle*)csv;
    return h && h->magic == kCsvMagic ? h : nullptr;
}

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// The index of h->d_bytes into h; stats8 is filled on success.
int open_run(CsvHandle& h, uint64_t* stats8, hipStream_t st) {
    using namespace oxh;
    const uint64_t n = h.nbytes, mis = (uintptr_t)h.d_bytes & 15, lo = mis, hi = mis + n;
    const uint8_t* base = h.d_bytes - mis;
    const uint64_t tiles = csv::tiles_of(mis, n);
    if (csv::scan_tiles_of(tiles) != scan_tiles(tiles)) return fail(OXH_ERR_HIP, "csv: the scan's tile is not the lease's");
    unsigned long long inside = 0;
    {
        const csv::IndexLease at(tiles);
        ScratchLease lease(st);  // ends (and waits for the stream) with this block
        void* lbase = nullptr;
        void* pinned = nullptr;
        if (lease.get(at.total, &lbase) != hipSuccess || lease.pinned(csv::kCtrlBytes, &pinned) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "csv: " + std::to_string(at.total) + " B of tile counts and their scans");
        }
        uint8_t* b = (uint8_t*)lbase;
        unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
        unsigned long long* h_ctrl = (unsigned long long*)pinned;
        uint32_t *d_quotes = (uint32_t*)(b + at.quotes), *d_delims = (uint32_t*)(b + at.delims), *d_recs = (uint32_t*)(b + at.recs);
        uint64_t *d_qscan = (uint64_t*)(b + at.quote_scan), *d_dscan = (uint64_t*)(b + at.delim_scan), *d_rscan = (uint64_t*)(b + at.rec_scan);
        unsigned long long *d_qsums = (unsigned long long*)(b + at.quote_sums), *d_dsums = (unsigned long long*)(b + at.delim_sums),
                           *d_rsums = (unsigned long long*)(b + at.rec_sums);
        const unsigned grid = cap_grid(tiles);
        const uint64_t last = scan_tiles(tiles);
        int rc = [&]() -> int {
            HIP_TRY(hipMemsetAsync(d_ctrl, 0, kCsvCtrlWords * 8, st));
            csv_classify_kernel<<<grid, 256, 0, st>>>(base, lo, hi, h.sep, h.quote, tiles, d_quotes);
            HIP_TRY(hipGetLastError());
            int r = exclusive_scan_u32(d_quotes, tiles, d_qscan, d_qsums, st);
            if (r) return r;
            csv_delims_kernel<false><<<grid, 256, 0, st>>>(base, lo, hi, h.sep, h.quote, tiles, d_qscan, d_delims, d_recs, nullptr, nullptr,
                                                           nullptr, nullptr, 0, 0, d_ctrl);
            HIP_TRY(hipGetLastError());
            if ((r = exclusive_scan_u32(d_delims, tiles, d_dscan, d_dsums, st))) return r;
            if ((r = exclusive_scan_u32(d_recs, tiles, d_rscan, d_rsums, st))) return r;
            HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, kCsvCtrlWords * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_ctrl + kCsvCtrlWords, d_dsums + last, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_ctrl + kCsvCtrlWords + 1, d_rsums + last, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            h.nends = h_ctrl[kCsvCtrlWords], h.nrec = h_ctrl[kCsvCtrlWords + 1];
            inside = h_ctrl[kCsvCtrlInside];
            if (h.nrec == 0 || h.nends < h.nrec || h.nends > n + 1) return fail(OXH_ERR_HIP, "csv: the delimiter counts are not those of a buffer (did it change during the call?)");
            const uint64_t words = h.nends + 2 * h.nrec;
            if (hipMalloc(&h.block, words * 4) != hipSuccess) {
                (void)hipGetLastError();
                h.block = nullptr;
                return fail(OXH_ERR_NOMEM, "csv: " + std::to_string(words * 4) + " B for the index");
            }
            poison_device(h.block, words * 4, st);
            h.ends = h.block, h.rec_end = h.block + h.nends, h.row_rec = h.rec_end + h.nrec;
            csv_delims_kernel<true><<<grid, 256, 0, st>>>(base, lo, hi, h.sep, h.quote, tiles, d_qscan, nullptr, nullptr, d_dscan, d_rscan, h.ends,
                                                          h.rec_end, h.nends, h.nrec, d_ctrl);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h_ctrl[kCsvCtrlErr]) return fail(OXH_ERR_HIP, "csv: a delimiter's place is outside the index (did the buffer change during the call?)");
            return OXH_OK;
        }();
        if (rc != OXH_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    const uint64_t blocks = csv::blocks_of(h.nrec);
    if (csv::scan_tiles_of(blocks) != scan_tiles(blocks)) return fail(OXH_ERR_HIP, "csv: the scan's tile is not the lease's");
    const csv::RowMapLease at(h.nrec);
    ScratchLease lease(st);
    void* lbase = nullptr;
    void* pinned = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess || lease.pinned(csv::kCtrlBytes, &pinned) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "csv: " + std::to_string(at.total) + " B of record masks and their scan");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    unsigned long long* h_ctrl = (unsigned long long*)pinned;
    uint64_t *d_mask = (uint64_t*)(b + at.mask), *d_bases = (uint64_t*)(b + at.bases);
    uint32_t* d_counts = (uint32_t*)(b + at.counts);
    unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
    const uint32_t hdr = h.flags & OXH_CSV_HAS_HEADER ? 1 : 0;
    std::vector<uint32_t> hdr_ends;
    std::vector<uint8_t> hdr_bytes;
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kCsvCtrlWords * 8, st));
        csv_keep_kernel<<<row_grid(h.nrec), 256, 0, st>>>(h.d_bytes, h.ends, h.rec_end, h.nrec, d_mask, d_counts);
        HIP_TRY(hipGetLastError());
        int r = exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st);
        if (r) return r;
        csv_rowmap_kernel<<<row_grid(h.nrec), 256, 0, st>>>(d_mask, d_bases, h.nrec, h.row_rec, d_ctrl);
        HIP_TRY(hipGetLastError());
        csv_shape_kernel<<<row_grid(h.nrec), 256, 0, st>>>(h.ends, h.rec_end, h.row_rec, d_sums + scan_tiles(blocks), hdr, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, kCsvCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ctrl + kCsvCtrlWords, d_sums + scan_tiles(blocks), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_ctrl[kCsvCtrlErr]) return fail(OXH_ERR_HIP, "csv: a kept record's place is outside the row map (did the buffer change during the call?)");
        h.nkept = h_ctrl[kCsvCtrlWords];
        h.ncols = h_ctrl[kCsvCtrlNcols];
        if (h.nkept > h.nrec || (h.nkept && (h.ncols == 0 || h_ctrl[kCsvCtrlHdrFirst] + h.ncols > h.nends)))
            return fail(OXH_ERR_HIP, "csv: the row map is not that of the index");
        h.nrows = h.nkept - (hdr && h.nkept ? 1 : 0);
        if (hdr && h.nkept) {  // the header record comes down: its fields' ends and its bytes
            const uint64_t first = h_ctrl[kCsvCtrlHdrFirst], start = h_ctrl[kCsvCtrlHdrStart];
            hdr_ends.resize(h.ncols);
            HIP_TRY(hipMemcpyAsync(hdr_ends.data(), h.ends + first, h.ncols * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint64_t end = hdr_ends.back();
            if (end < start || end > n) return fail(OXH_ERR_HIP, "csv: the header record is not inside the buffer");
            hdr_bytes.resize(end - start + 1);
            if (end > start) {
                HIP_TRY(hipMemcpyAsync(hdr_bytes.data(), h.d_bytes + start, end - start, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            csv::header_names(hdr_bytes.data(), (uint32_t)start, hdr_ends.data(), (uint32_t)h.ncols, h.quote, h.names, h.name_offsets);
        }
        return OXH_OK;
    }();
    if (rc != OXH_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    stats8[0] = h.nrec, stats8[1] = h.nrows, stats8[2] = h.ncols, stats8[3] = h.nends, stats8[4] = h.nrec - h.nkept;
    stats8[5] = h_ctrl[kCsvCtrlShort], stats8[6] = h_ctrl[kCsvCtrlLong], stats8[7] = inside;
    STEP("csv open: %llu B, %llu records, %llu rows x %llu columns", (unsigned long long)n, (unsigned long long)h.nrec,
         (unsigned long long)h.nrows, (unsigned long long)h.ncols);
    return OXH_OK;
}

int open_enter(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint32_t separator, uint32_t quote, uint32_t flags, void** out,
               uint64_t* stats8, bool& done) {
    done = false;
    const std::string what = csv::open_error(bytes, nbytes, separator, quote, flags, out, stats8);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "csv open: " + what);
    if (nbytes == 0) {  // a valid empty handle: no records, no columns
        CsvHandle* h = new CsvHandle;
        h->ctx = ctx, h->sep = separator, h->quote = quote, h->flags = flags;
        memset(stats8, 0, 8 * sizeof(uint64_t));
        *out = h;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

struct Selection {
    uint32_t nsel;
    const uint32_t* col_idx;
    const uint32_t* types;
};

// The measure: for every string column (and, with `all`, every other one) ctrl[k * kColWords ..] on the host.
int columns_measure(CsvHandle& h, const Selection& s, bool all, std::vector<unsigned long long>& ctrl, hipStream_t st) {
    using namespace oxh;
    const CsvView v = h.view();
    ctrl.assign((size_t)s.nsel * kColWords, 0);
    ScratchLease lease(st);
    void* lbase = nullptr;
    const uint64_t bytes = (uint64_t)s.nsel * kColWords * 8;
    if (lease.get(csv::align256(bytes), &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "csv columns: " + std::to_string(bytes) + " B of control words");
    }
    unsigned long long* d_ctrl = (unsigned long long*)lbase;
    const unsigned grid = row_grid(h.nrows);
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, bytes, st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            unsigned long long* c = d_ctrl + (size_t)k * kColWords;
            const uint32_t col = s.col_idx[k];
            if (csv::is_string(s.types[k]))
                csv_str_len_kernel<<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, c);
            else if (!all)
                continue;
            else if (s.types[k] == OXH_CSV_INT64)
                csv_fixed_kernel<OXH_CSV_INT64><<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, nullptr, nullptr, nullptr, c);
            else if (s.types[k] == OXH_CSV_FLOAT64)
                csv_fixed_kernel<OXH_CSV_FLOAT64><<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, nullptr, nullptr, nullptr, c);
            else
                csv_fixed_kernel<OXH_CSV_BOOL><<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, nullptr, nullptr, nullptr, c);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(ctrl.data(), d_ctrl, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// The deferred cells of one FLOAT64 column (`ndeferred` of them; their masks and counts are written): compacted,
// brought down, converted, scattered into d_values.
int convert_deferred(CsvHandle& h, uint32_t col, uint64_t ndeferred, const uint64_t* d_mask, const uint32_t* d_counts, uint64_t* d_bases,
                     unsigned long long* d_sums, unsigned long long* d_ctrl, uint64_t* d_values, hipStream_t st) {
    using namespace oxh;
    const CsvView v = h.view();
    const uint64_t blocks = csv::blocks_of(h.nrows);
    const uint64_t list_bytes = csv::align256(ndeferred * 12), slot_bytes = csv::align256(ndeferred * kCsvDeferSlot), value_bytes = ndeferred * 8;
    uint8_t* block = nullptr;
    if (hipMalloc(&block, list_bytes + slot_bytes + value_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "csv columns: " + std::to_string(list_bytes + slot_bytes + value_bytes) + " B for the deferred cells");
    }
    poison_device(block, list_bytes + slot_bytes + value_bytes, st);
    uint32_t* d_list = (uint32_t*)block;
    uint8_t* d_slots = block + list_bytes;
    uint64_t* d_converted = (uint64_t*)(block + list_bytes + slot_bytes);
    std::vector<uint32_t> list(ndeferred * 3);
    std::vector<uint8_t> slots(ndeferred * kCsvDeferSlot);
    std::vector<uint64_t> converted(ndeferred);
    uint8_t* long_block = nullptr;  // the jobs and the bytes of the texts longer than a slot, where there are any
    int rc = [&]() -> int {
        int r = exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st);
        if (r) return r;
        csv_defer_emit_kernel<<<row_grid(h.nrows), 256, 0, st>>>(v, col, d_mask, d_bases, ndeferred, d_list, d_slots, d_ctrl);
        HIP_TRY(hipGetLastError());
        unsigned long long err = 0;
        HIP_TRY(hipMemcpyAsync(list.data(), d_list, list.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(slots.data(), d_slots, slots.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&err, d_ctrl + kColErr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (err) return fail(OXH_ERR_HIP, "csv columns: a deferred cell's place is outside the list (did the buffer change during the call?)");
        // the texts longer than a slot (hundreds of digits): gathered by one launch, brought down by one copy
        std::vector<uint64_t> jobs;  // per long text: where it starts | its length << 32, then its place in `text`
        uint64_t long_bytes = 0;
        for (uint64_t k = 0; k < ndeferred; ++k) {
            const uint32_t start = list[3 * k + 1], len = list[3 * k + 2];
            if ((uint64_t)start + len > h.nbytes) return fail(OXH_ERR_HIP, "csv columns: a deferred cell is not inside the buffer");
            if (len <= kCsvDeferSlot) continue;
            jobs.push_back(start | (uint64_t)len << 32), jobs.push_back(long_bytes);
            long_bytes += len;
        }
        std::vector<char> text(long_bytes);
        if (!jobs.empty()) {
            const uint64_t job_bytes = jobs.size() * 8;
            if (hipMalloc(&long_block, job_bytes + long_bytes) != hipSuccess) {
                (void)hipGetLastError();
                long_block = nullptr;
                return fail(OXH_ERR_NOMEM, "csv columns: " + std::to_string(job_bytes + long_bytes) + " B for the long deferred texts");
            }
            poison_device(long_block, job_bytes + long_bytes, st);
            HIP_TRY(hipMemcpyAsync(long_block, jobs.data(), job_bytes, hipMemcpyHostToDevice, st));
            csv_defer_long_kernel<<<cap_grid((jobs.size() / 2 + 3) / 4), 256, 0, st>>>(h.d_bytes, (const uint64_t*)long_block, jobs.size() / 2,
                                                                                        long_block + job_bytes);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(text.data(), long_block + job_bytes, long_bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        uint64_t long_at = 0;
        for (uint64_t k = 0; k < ndeferred; ++k) {
            const uint32_t len = list[3 * k + 2];
            const char* p = (const char*)slots.data() + k * kCsvDeferSlot;
            if (len > kCsvDeferSlot) p = text.data() + long_at, long_at += len;
            const double x = csv::convert_deferred(p, len);
            memcpy(&converted[k], &x, 8);
        }
        HIP_TRY(hipMemcpyAsync(d_converted, converted.data(), value_bytes, hipMemcpyHostToDevice, st));
        csv_defer_scatter_kernel<<<row_grid(ndeferred), 256, 0, st>>>(d_list, d_converted, ndeferred, h.nrows, d_values);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(block);
    if (long_block) (void)hipFree(long_block);
    return rc;
}

// Every selected column into the device buffers the tables name; string_bytes[k]: the measured bytes of a string
// column. ctrl: as columns_measure's.
int columns_write(CsvHandle& h, const Selection& s, const std::vector<uint64_t>& string_bytes, void* const* d_values, void* const* d_offsets,
                  uint8_t* const* d_validity, std::vector<unsigned long long>& ctrl, hipStream_t st) {
    using namespace oxh;
    const CsvView v = h.view();
    const uint64_t n = h.nrows;
    if (csv::scan_tiles_of(n) != scan_tiles(n)) return fail(OXH_ERR_HIP, "csv: the scan's tile is not the lease's");
    const csv::ColumnsLease at(n, s.nsel, s.types, true);
    ctrl.assign((size_t)s.nsel * kColWords, 0);
    ScratchLease lease(st);
    void* lbase = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "csv columns: " + std::to_string(at.total) + " B of lengths, their scan and the deferred masks");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    uint32_t* d_lens = (uint32_t*)(b + at.lens);
    uint64_t* d_len_scan = (uint64_t*)(b + at.len_scan);
    unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
    const uint64_t ctrl_bytes = (uint64_t)s.nsel * kColWords * 8;
    const unsigned grid = row_grid(n);
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, ctrl_bytes, st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            unsigned long long* c = d_ctrl + (size_t)k * kColWords;
            const uint32_t col = s.col_idx[k], type = s.types[k];
            if (csv::is_string(type)) {
                csv_str_len_kernel<<<grid, 256, 0, st>>>(v, col, d_lens, d_validity[k], c);
                HIP_TRY(hipGetLastError());
                int r = exclusive_scan_u32(d_lens, n, d_len_scan, d_sums, st);
                if (r) return r;
                csv_str_copy_kernel<<<grid, 256, 0, st>>>(v, col, d_lens, d_len_scan, string_bytes[k], d_offsets[k], type == OXH_CSV_STRING64,
                                                          (uint8_t*)d_values[k], c);
            } else if (type == OXH_CSV_INT64) {
                csv_fixed_kernel<OXH_CSV_INT64><<<grid, 256, 0, st>>>(v, col, (uint64_t*)d_values[k], nullptr, d_validity[k], nullptr, nullptr, c);
            } else if (type == OXH_CSV_FLOAT64) {
                csv_fixed_kernel<OXH_CSV_FLOAT64><<<grid, 256, 0, st>>>(v, col, (uint64_t*)d_values[k], nullptr, d_validity[k],
                                                                        (uint64_t*)(b + at.defer_mask[k]), (uint32_t*)(b + at.defer_counts[k]), c);
            } else {
                csv_fixed_kernel<OXH_CSV_BOOL><<<grid, 256, 0, st>>>(v, col, nullptr, (uint8_t*)d_values[k], d_validity[k], nullptr, nullptr, c);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(ctrl.data(), d_ctrl, ctrl_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            const unsigned long long* c = ctrl.data() + (size_t)k * kColWords;
            if (c[kColErr]) return fail(OXH_ERR_HIP, "csv columns: a string's place is outside its column's bytes (did the buffer change during the call?)");
            if (csv::is_string(s.types[k]) && c[kColBytes] != string_bytes[k]) return fail(OXH_ERR_HIP, "csv columns: a column's bytes are not those measured");
            if (s.types[k] == OXH_CSV_FLOAT64 && c[kColDeferred]) {
                int r = convert_deferred(h, s.col_idx[k], c[kColDeferred], (const uint64_t*)(b + at.defer_mask[k]), (const uint32_t*)(b + at.defer_counts[k]),
                                         (uint64_t*)(b + at.defer_bases), d_sums, d_ctrl + (size_t)k * kColWords, (uint64_t*)d_values[k], st);
                if (r) return r;
            }
        }
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

void fill_stats(const Selection& s, uint64_t nrows, const std::vector<unsigned long long>& ctrl, uint64_t* value_bytes, uint64_t* stats4) {
    using namespace oxh;
    for (uint32_t k = 0; k < s.nsel; ++k) {
        const unsigned long long* c = ctrl.data() + (size_t)k * kColWords;
        value_bytes[k] = csv::is_string(s.types[k]) ? c[kColBytes] : csv::fixed_value_bytes(s.types[k], nrows);
        stats4[4 * k] = c[kColEmpty], stats4[4 * k + 1] = c[kColBad], stats4[4 * k + 2] = c[kColDeferred], stats4[4 * k + 3] = value_bytes[k];
    }
}

// What both forms of oxh_csv_columns_* do first. `done`: nothing left to do.
int columns_enter(void* csv_handle, const csv::ColumnsArgs& a, CsvHandle*& h, bool& done) {
    done = false;
    h = handle_of(csv_handle);
    if (!h) return fail(OXH_ERR_INVALID, "csv columns: the handle is NULL or not a CSV handle");
    csv::ColumnsArgs full = a;
    full.nrows = h->nrows, full.ncols = h->ncols;
    const std::string what = csv::columns_error(full);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "csv columns: " + what);
    if (a.nsel == 0 || h->nrows == 0) {
        for (uint32_t k = 0; k < a.nsel; ++k) a.value_bytes[k] = 0;
        for (uint32_t k = 0; k < 4 * a.nsel; ++k) a.stats4[k] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(h->ctx);
}

// Measure, check the strings' bytes, and -- with outputs -- write. measured: the strings' bytes where the caller
// has measured (and checked) them already.
int columns_run(CsvHandle& h, const csv::ColumnsArgs& a, void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity,
                const uint64_t* capacity, hipStream_t st, const std::vector<uint64_t>* measured = nullptr) {
    const Selection s{a.nsel, a.col_idx, a.types};
    const bool write = d_values != nullptr;
    bool strings = false;
    for (uint32_t k = 0; k < a.nsel; ++k) strings |= csv::is_string(a.types[k]);
    std::vector<unsigned long long> ctrl((size_t)a.nsel * oxh::kColWords, 0);
    std::vector<uint64_t> string_bytes(a.nsel, 0);
    if (measured) {
        string_bytes = *measured;
    } else if (strings || !write) {
        int rc = columns_measure(h, s, !write, ctrl, st);
        if (rc) return rc;
        for (uint32_t k = 0; k < a.nsel; ++k) {
            if (!csv::is_string(a.types[k])) continue;
            string_bytes[k] = ctrl[(size_t)k * oxh::kColWords + oxh::kColBytes];
            const std::string what = csv::string_bytes_error(a.types[k], string_bytes[k], write, write ? capacity[k] : 0);
            if (!what.empty()) return fail(OXH_ERR_INVALID, "csv columns: selection " + std::to_string(k) + ": " + what);
        }
    }
    if (write) {
        int rc = columns_write(h, s, string_bytes, d_values, d_offsets, d_validity, ctrl, st);
        if (rc) return rc;
    }
    fill_stats(s, h.nrows, ctrl, a.value_bytes, a.stats4);
    return OXH_OK;
}

}  // namespace

extern "C" {

int oxh_csv_open_device(oxh_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, uint32_t separator, uint32_t quote, uint32_t flags, void** out,
                        uint64_t* stats8, void* stream) {
    bool done = false;
    int rc = open_enter(ctx, d_bytes, nbytes, separator, quote, flags, out, stats8, done);
    if (rc || done) return rc;
    std::unique_ptr<CsvHandle> h(new CsvHandle);
    h->ctx = ctx, h->device = ctx->device, h->d_bytes = d_bytes, h->nbytes = nbytes, h->sep = separator, h->quote = quote, h->flags = flags;
    uint64_t stats[8] = {};
    rc = open_run(*h, stats, (hipStream_t)stream);
    if (rc) return rc;
    memcpy(stats8, stats, sizeof stats);
    *out = h.release();
    return OXH_OK;
}

int oxh_csv_open_host(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint32_t separator, uint32_t quote, uint32_t flags, void** out,
                      uint64_t* stats8) {
    bool done = false;
    int rc = open_enter(ctx, bytes, nbytes, separator, quote, flags, out, stats8, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    std::unique_ptr<CsvHandle> h(new CsvHandle);
    h->ctx = ctx, h->device = ctx->device, h->nbytes = nbytes, h->sep = separator, h->quote = quote, h->flags = flags;
    // the copy keeps the caller's phase within 16 bytes: the aligned loads fall where they would on the caller's buffer
    const uint64_t phase = (uintptr_t)bytes & 15;
    if (hipMalloc(&h->owned, nbytes + 32) != hipSuccess) {
        (void)hipGetLastError();
        h->owned = nullptr;
        return fail(OXH_ERR_NOMEM, "csv open: " + std::to_string(nbytes) + " B for the file on the device");
    }
    oxh::poison_device(h->owned, nbytes + 32, st);
    h->d_bytes = h->owned + phase;
    HIP_TRY(hipMemcpyAsync(h->owned + phase, bytes, nbytes, hipMemcpyHostToDevice, st));
    uint64_t stats[8] = {};
    rc = open_run(*h, stats, st);
    if (rc) return rc;
    memcpy(stats8, stats, sizeof stats);
    *out = h.release();
    return OXH_OK;
}

int oxh_csv_close(void* csv_handle) {
    if (!csv_handle) return OXH_OK;
    CsvHandle* h = handle_of(csv_handle);
    if (!h) return fail(OXH_ERR_INVALID, "csv close: not a CSV handle");
    if (h->block || h->owned) (void)hipSetDevice(h->device);
    delete h;
    return OXH_OK;
}

int oxh_csv_header(void* csv_handle, uint8_t* names, uint64_t capacity, uint64_t* name_offsets, uint64_t* names_bytes) {
    CsvHandle* h = handle_of(csv_handle);
    if (!h) return fail(OXH_ERR_INVALID, "csv header: the handle is NULL or not a CSV handle");
    if (!name_offsets || !names_bytes) return fail(OXH_ERR_INVALID, "csv header: name_offsets or names_bytes is NULL");
    *names_bytes = h->names.size();
    if (!names || capacity < h->names.size()) return OXH_OK;
    if (!h->names.empty()) memcpy(names, h->names.data(), h->names.size());
    for (uint64_t c = 0; c <= h->ncols; ++c) name_offsets[c] = c < h->name_offsets.size() ? h->name_offsets[c] : 0;
    return OXH_OK;
}

int oxh_csv_infer(void* csv_handle, uint64_t max_rows, uint32_t* types) {
    using namespace oxh;
    CsvHandle* h = handle_of(csv_handle);
    if (!h) return fail(OXH_ERR_INVALID, "csv infer: the handle is NULL or not a CSV handle");
    if (h->ncols && !types) return fail(OXH_ERR_INVALID, "csv infer: types is NULL");
    const uint64_t rows = std::min(max_rows, h->nrows), ncols = h->ncols;
    if (!rows) {
        for (uint64_t c = 0; c < ncols; ++c) types[c] = OXH_CSV_STRING;
        return OXH_OK;
    }
    int rc = device_enter(h->ctx);
    if (rc) return rc;
    hipStream_t st = h->ctx->stream;
    std::vector<uint32_t> words(2 * ncols);
    {
        ScratchLease lease(st);
        void* lbase = nullptr;
        if (lease.get(csv::align256(ncols * 8), &lbase) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "csv infer: " + std::to_string(ncols * 8) + " B of class bits");
        }
        uint32_t* d_bits = (uint32_t*)lbase;
        rc = [&]() -> int {
            HIP_TRY(hipMemsetAsync(d_bits, 0xFF, ncols * 4, st));
            HIP_TRY(hipMemsetAsync(d_bits + ncols, 0, ncols * 4, st));
            csv_infer_kernel<<<row_grid(rows), 256, 0, st>>>(h->view(), rows, (uint32_t)ncols, d_bits, d_bits + ncols);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(words.data(), d_bits, ncols * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return OXH_OK;
        }();
        if (rc != OXH_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    for (uint64_t c = 0; c < ncols; ++c) types[c] = csv::type_of_bits(words[c] & csvnum::kAllOk, words[ncols + c] == 0);
    return OXH_OK;
}

int oxh_csv_columns_device(void* csv_handle, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                           void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity, uint64_t* value_bytes, uint64_t* stats4,
                           void* stream) {
    const csv::ColumnsArgs a{0, 0, nsel, col_idx, types, value_capacity, d_values, d_offsets, d_validity, value_bytes, stats4};
    CsvHandle* h = nullptr;
    bool done = false;
    int rc = columns_enter(csv_handle, a, h, done);
    if (rc || done) return rc;
    return columns_run(*h, a, d_values, d_offsets, d_validity, value_capacity, (hipStream_t)stream);
}

int oxh_csv_columns_host(void* csv_handle, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                         void* const* values, void* const* offsets, uint8_t* const* validity, uint64_t* value_bytes, uint64_t* stats4) {
    const csv::ColumnsArgs a{0, 0, nsel, col_idx, types, value_capacity, values, offsets, validity, value_bytes, stats4};
    CsvHandle* h = nullptr;
    bool done = false;
    int rc = columns_enter(csv_handle, a, h, done);
    if (rc || done) return rc;
    hipStream_t st = h->ctx->stream;
    if (!values) return columns_run(*h, a, nullptr, nullptr, nullptr, nullptr, st);
    // the strings' bytes first, and only theirs: the device block holds exactly what the columns need
    std::vector<uint64_t> bytes(nsel, 0);
    bool strings = false;
    for (uint32_t k = 0; k < nsel; ++k) strings |= csv::is_string(types[k]);
    if (strings) {
        std::vector<unsigned long long> ctrl;
        rc = columns_measure(*h, Selection{nsel, col_idx, types}, false, ctrl, st);
        if (rc) return rc;
        for (uint32_t k = 0; k < nsel; ++k)
            if (csv::is_string(types[k])) bytes[k] = ctrl[(size_t)k * oxh::kColWords + oxh::kColBytes];
    }
    const uint64_t n = h->nrows, bitmap = (n + 7) / 8;
    for (uint32_t k = 0; k < nsel; ++k)
        if (!csv::is_string(types[k])) bytes[k] = csv::fixed_value_bytes(types[k], n);
    std::vector<uint64_t> at_values(nsel), at_offsets(nsel), at_validity(nsel), offset_bytes(nsel, 0);
    uint64_t total = 0;
    auto carve = [&](uint64_t b) {
        const uint64_t here = total;
        total += (b + 15) & ~15ull;
        return here;
    };
    for (uint32_t k = 0; k < nsel; ++k) {
        if (csv::is_string(types[k])) {
            const std::string what = csv::string_bytes_error(types[k], bytes[k], true, value_capacity[k]);
            if (!what.empty()) return fail(OXH_ERR_INVALID, "csv columns: selection " + std::to_string(k) + ": " + what);
            offset_bytes[k] = (n + 1) * (types[k] == OXH_CSV_STRING64 ? 8 : 4);
        }
        at_values[k] = carve(bytes[k]), at_offsets[k] = carve(offset_bytes[k]), at_validity[k] = carve(bitmap);
    }
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "csv columns: " + std::to_string(total) + " B for the columns on the device");
    }
    oxh::poison_device(d_block, total + 16, st);
    std::vector<void*> d_values(nsel), d_offsets(nsel);
    std::vector<uint8_t*> d_validity(nsel);
    for (uint32_t k = 0; k < nsel; ++k)
        d_values[k] = d_block + at_values[k], d_offsets[k] = d_block + at_offsets[k], d_validity[k] = d_block + at_validity[k];
    rc = [&]() -> int {
        int r = columns_run(*h, a, d_values.data(), d_offsets.data(), d_validity.data(), bytes.data(), st, &bytes);
        if (r) return r;
        // the caller's arrays stay untouched unless everything succeeded
        for (uint32_t k = 0; k < nsel; ++k) {
            if (bytes[k]) HIP_TRY(hipMemcpyAsync(values[k], d_values[k], bytes[k], hipMemcpyDeviceToHost, st));
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
