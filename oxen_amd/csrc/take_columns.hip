// oxen_amd/csrc/take_columns.hip -- the columns of the joined rows of a keyed diff (oxh_take_columns_*): a
// take (gather by row index) of Arrow columns with null indices and an optional fallback source. The
// reference builds TabularDiff.contents with polars on the host (repositories/diffs/join_diff.rs: the full
// join :290, `coalesce(key.right, key.left)` :95-102, `select(output_columns)` :134); here the two frames'
// columns and the pairs of oxh_keyed_diff_* stay on the device and one call writes the output columns as
// Arrow buffers that start at bit / offset 0 (DESIGN.md §4 "Take").
//
// Output row i reads its two indices once; cell (o, i) is the cell of column a at idx[ia][i] when that
// index is present and the cell valid, else the same through (b, ib), else null. One call is, on one stream:
//   measure   (only with byte output columns) take_resolve_kernel<false>: one lane per output row resolves
//             every byte column's cell and stores its length (u32, leased from scratch.hpp); the cells
//             longer than the short / long threshold and their pieces of at most kTakePiece bytes are
//             counted per wave, per workgroup, one atomic each;
//   scan      exclusive_scan_u32 over each byte column's lengths: the output offsets, the total in the
//             scan's last word. One read-back brings the totals, the counts and the error word: the
//             sizes-only call and the call whose bytes do not fit stop here, no output touched;
//   write     take_resolve_kernel<true>, row = global thread index, so a wave owns rows [64w, 64w + 64):
//             a fixed-width cell is one gathered load and one coalesced store (0 for a null); validity and
//             boolean bits are a ballot per wave, one lane stores the wave's 64-bit word (the last wave its
//             ceil(rem / 8) bytes singly); a byte column's lane writes the row's offset in the column's
//             width and copies a short cell itself, 8 then 4 then 1 byte at a time;
//   long      take_long_plan_kernel lists the long cells as (row, column, piece) items -- a prefix sum of
//             the pieces inside the workgroup on top of one atomic add per workgroup -- and
//             take_long_gather_kernel copies one item per wave, 8 bytes per lane and step.
// There are no atomics and no read-modify-write on any output. No lane waits for another lane or workgroup.
// An index that is neither absent nor below its column's rows is a null cell and sets the error word, as a
// decreasing or negative pair of offsets does (row_cell); a destination outside the scanned total and a
// list place outside the counted pieces are never written.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "take_columns_host.hpp"

using namespace oxh::capi;

namespace oxh {

// The short / long threshold and the piece size (tools/take_probe.py swept both: DESIGN.md §4 "Take").
constexpr uint32_t kTakeShortMax = 256;
constexpr uint32_t kTakePiece = 4096;
constexpr uint32_t kTakeNone = OXH_TAKE_NULL;
// beside kRowErrOffsets, kRowErrValues (columns.hpp)
constexpr unsigned long long kTakeErrIndex = 4, kTakeErrPlace = 8, kTakeErrLength = 16;
// ctrl words of one call: the error word, the long cells, their pieces, the plan's cursor
constexpr int kTakeCtrlErr = 0, kTakeCtrlLong = 1, kTakeCtrlPieces = 2, kTakeCtrlCursor = 3, kTakeCtrlWords = 4;

struct TakeSrc {
    RowCol col;
    uint64_t rows;
};

struct TakeOut {
    uint8_t *values, *offsets, *validity;  // the caller's buffers (write pass)
    uint32_t* len;                         // byte columns: every row's resolved cell length,
    const uint64_t* off;                   // their exclusive prefix sums
    const unsigned long long* total;       // and their sum
    uint32_t a, ia, b, ib;                 // the plan entry
    uint32_t kind, pad;
};

struct TakeArgs {
    const TakeSrc* src;
    const TakeOut* out;
    const uint32_t *idx0, *idx1;  // NULL: all absent
    uint64_t n;                   // output rows
    uint32_t nout, short_max, piece, pad;
    unsigned long long* ctrl;
    uint32_t* item_row;           // the long cells' pieces: output row,
    uint64_t* item_cp;            // output column << 32 | piece
    uint64_t nitems;
};

__device__ __forceinline__ bool take_is_bytes(uint32_t kind) { return kind == OXH_COL_BYTES32 || kind == OXH_COL_BYTES64; }

// Is the cell of source column `col` at row r there? Nothing is read through an index that is no row.
__device__ __forceinline__ bool take_from(const TakeArgs& a, uint32_t col, uint32_t r, unsigned long long& bad) {
    if (r == kTakeNone) return false;
    const TakeSrc& s = a.src[col];
    if (r >= s.rows) {
        bad |= kTakeErrIndex;
        return false;
    }
    return !s.col.validity || row_bit(s.col.validity, s.col.nbit + r);
}

// Where cell (o, i) comes from: false = null.
__device__ __forceinline__ bool take_source(const TakeArgs& a, const TakeOut& o, uint32_t i0, uint32_t i1, uint32_t& col,
                                            uint32_t& row, unsigned long long& bad) {
    uint32_t r = o.ia ? i1 : i0;
    if (take_from(a, o.a, r, bad)) {
        col = o.a, row = r;
        return true;
    }
    if (o.b == OXH_TAKE_NO_COLUMN) return false;
    r = o.ib ? i1 : i0;
    if (take_from(a, o.b, r, bad)) {
        col = o.b, row = r;
        return true;
    }
    return false;
}

// The bytes of a byte column's cell: its length, `start` = where they begin in the column's values.
__device__ __forceinline__ uint32_t take_span(const TakeArgs& a, uint32_t col, uint32_t row, uint64_t& start,
                                              unsigned long long& bad) {
    const uint64_t len = row_cell(a.src[col].col, row, start, bad);
    if (len > 0xFFFFFFFFull) {  // the lengths are u32
        bad |= kTakeErrLength;
        return 0;
    }
    return (uint32_t)len;
}

// The wave's 64 bits of a bit-packed output (the rows from wave_row0 on): one lane stores the word; the last
// wave stores only the bytes that hold its rows, a lane each. A lane past the last row has contributed 0.
__device__ __forceinline__ void take_store_bits(uint8_t* dst, uint64_t wave_row0, uint64_t n, unsigned lane,
                                                unsigned long long word) {
    if (wave_row0 >= n) return;
    uint8_t* at = dst + (wave_row0 >> 3);
    if (wave_row0 + 64 <= n) {
        if (lane == 0) *reinterpret_cast<unsigned long long*>(at) = word;
    } else if (lane < ((n - wave_row0 + 7) >> 3)) {
        at[lane] = (uint8_t)(word >> (8 * lane));
    }
}

// WRITE false: the lengths of the byte columns' cells, and the long cells and their pieces counted.
// WRITE true: every output but the bytes of the long cells. Row = global thread index; every lane of a wave
// reaches the ballots (nothing returns early).
template <bool WRITE>
__global__ __launch_bounds__(256) void take_resolve_kernel(TakeArgs a) {
    __shared__ unsigned long long part[4][2];
    const unsigned lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t wave_row0 = i - lane;
    const bool live = i < a.n;
    const uint32_t i0 = live && a.idx0 ? a.idx0[i] : kTakeNone;
    const uint32_t i1 = live && a.idx1 ? a.idx1[i] : kTakeNone;
    unsigned long long bad = 0, nlong = 0, npieces = 0;
    for (uint32_t k = 0; k < a.nout; ++k) {
        TakeOut o = a.out[k];  // the same for every lane
        o.kind = __builtin_amdgcn_readfirstlane(o.kind);  // and known to be: the ballots below are under no divergent branch
        const bool bytes = take_is_bytes(o.kind);
        if (!WRITE && !bytes) continue;
        uint32_t col = 0, row = 0;
        const bool has = live && take_source(a, o, i0, i1, col, row, bad);
        if (bytes) {
            uint64_t start = 0;
            const uint32_t len = has ? take_span(a, col, row, start, bad) : 0;
            if constexpr (!WRITE) {
                if (live) o.len[i] = len;
                if (len > a.short_max) {
                    nlong += 1;
                    npieces += ((uint64_t)len + a.piece - 1) / a.piece;
                }
            } else if (live) {
                const uint64_t at = o.off[i], total = *o.total;
                if (at > total || len > total - at) {  // not what the measure pass saw: never past the scanned total
                    bad |= kTakeErrPlace;
                } else {
                    if (o.kind == OXH_COL_BYTES32) {
                        reinterpret_cast<int32_t*>(o.offsets)[i] = (int32_t)at;
                        if (i + 1 == a.n) reinterpret_cast<int32_t*>(o.offsets)[i + 1] = (int32_t)(at + len);
                    } else {
                        reinterpret_cast<int64_t*>(o.offsets)[i] = (int64_t)at;
                        if (i + 1 == a.n) reinterpret_cast<int64_t*>(o.offsets)[i + 1] = (int64_t)(at + len);
                    }
                    if (len && len <= a.short_max) {  // exactly the len bytes of the span, the widest pieces first
                        const uint8_t* src = a.src[col].col.values + start;
                        uint8_t* dst = o.values + at;
                        uint32_t b = 0;
                        for (; b + 8 <= len; b += 8) {
                            const uint64_t v = ld64u(src + b);
                            __builtin_memcpy(dst + b, &v, 8);
                        }
                        if (b + 4 <= len) {
                            const uint32_t v = ld32u(src + b);
                            __builtin_memcpy(dst + b, &v, 4);
                            b += 4;
                        }
                        for (; b < len; ++b) dst[b] = src[b];
                    }
                }
            }
        } else if constexpr (WRITE) {
            const RowCol& c = a.src[col].col;  // column 0 when the cell is null: not read then
            switch (o.kind) {
                case OXH_COL_FIXED1:
                    if (live) o.values[i] = has ? c.values[row] : 0;
                    break;
                case OXH_COL_FIXED4: {
                    const uint32_t v = has ? ld32u(c.values + 4ull * row) : 0;
                    if (live) __builtin_memcpy(o.values + 4 * i, &v, 4);
                    break;
                }
                case OXH_COL_FIXED8: {
                    const uint64_t v = has ? ld64u(c.values + 8ull * row) : 0;
                    if (live) __builtin_memcpy(o.values + 8 * i, &v, 8);
                    break;
                }
                default:  // OXH_COL_BOOL
                    take_store_bits(o.values, wave_row0, a.n, lane, __ballot(has && row_bit(c.values, c.vbit + row)));
                    break;
            }
        }
        if constexpr (WRITE) take_store_bits(o.validity, wave_row0, a.n, lane, __ballot(has));
    }
    if (bad) __hip_atomic_fetch_or(&a.ctrl[kTakeCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (!WRITE) {
        // every lane is here
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            nlong += (unsigned long long)__shfl_xor((long long)nlong, off, 64);
            npieces += (unsigned long long)__shfl_xor((long long)npieces, off, 64);
        }
        if (lane == 0) part[threadIdx.x >> 6][0] = nlong, part[threadIdx.x >> 6][1] = npieces;
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
            if (sum) atomicAdd(&a.ctrl[kTakeCtrlLong + threadIdx.x], sum);
        }
    }
}

// (the lengths are stored) Every piece of every long cell gets a place in the item lists: an exclusive prefix
// sum of the rows' piece counts over the workgroup -- shuffles in the wave, the four wave totals through LDS
// -- on top of what one atomic add per workgroup returns. Which workgroup's items come first is not fixed;
// an item says where its bytes go, so the result is.
__global__ __launch_bounds__(256) void take_long_plan_kernel(TakeArgs a) {
    __shared__ unsigned long long wave_sum[4], wave_base[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine = 0;
    if (i < a.n)
        for (uint32_t k = 0; k < a.nout; ++k) {
            if (!take_is_bytes(a.out[k].kind)) continue;
            const uint32_t len = a.out[k].len[i];
            if (len > a.short_max) mine += ((uint64_t)len + a.piece - 1) / a.piece;
        }
    unsigned long long incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, off, 64);
        if (lane >= (unsigned)off) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < 4; ++w) {
            wave_base[w] = sum;
            sum += wave_sum[w];
        }
        const unsigned long long first = sum ? atomicAdd(&a.ctrl[kTakeCtrlCursor], sum) : 0;
        for (int w = 0; w < 4; ++w) wave_base[w] += first;
    }
    __syncthreads();
    if (!mine) return;
    uint64_t at = wave_base[wave] + (incl - mine);
    for (uint32_t k = 0; k < a.nout; ++k) {
        if (!take_is_bytes(a.out[k].kind)) continue;
        const uint32_t len = a.out[k].len[i];
        if (len <= a.short_max) continue;
        const uint32_t pieces = (uint32_t)(((uint64_t)len + a.piece - 1) / a.piece);
        for (uint32_t p = 0; p < pieces; ++p, ++at) {
            if (at >= a.nitems) {  // more than the measure pass counted
                __hip_atomic_fetch_or(&a.ctrl[kTakeCtrlErr], kTakeErrPlace, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            a.item_row[at] = (uint32_t)i;
            a.item_cp[at] = (uint64_t)k << 32 | p;
        }
    }
}

// One wave per item: at most a.piece bytes of one long cell, 8 bytes per lane and step, to their place in
// the output column's values. (The lists were 0xFF-filled: an entry the plan did not fill names no row.)
__global__ __launch_bounds__(256) void take_long_gather_kernel(TakeArgs a) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.nitems) return;  // the whole wave
    const uint64_t i = a.item_row[w], cp = a.item_cp[w];
    const uint32_t k = (uint32_t)(cp >> 32), piece = (uint32_t)cp;
    if (i >= a.n || k >= a.nout) return;
    const TakeOut o = a.out[k];
    if (!take_is_bytes(o.kind)) return;
    unsigned long long bad = 0;
    uint32_t col = 0, row = 0;
    uint64_t start = 0;
    const bool has = take_source(a, o, a.idx0 ? a.idx0[i] : kTakeNone, a.idx1 ? a.idx1[i] : kTakeNone, col, row, bad);
    const uint32_t len = has ? take_span(a, col, row, start, bad) : 0;
    const uint64_t at = o.off[i], total = *o.total, begin = (uint64_t)piece * a.piece;
    if (len <= a.short_max || begin >= len || at > total || len > total - at) {  // not the cell the plan listed
        bad |= kTakeErrPlace;
    } else {
        const uint64_t n = len - begin < a.piece ? len - begin : a.piece;
        const uint8_t* src = a.src[col].col.values + start + begin;
        uint8_t* dst = o.values + at + begin;
        // whole 8-byte pieces across the lanes (512 B per wave-instruction, any alignment), then the last
        // n % 8 bytes one lane each: exactly the n bytes
        const uint64_t whole = n & ~7ull;
        for (uint64_t b = 8ull * lane; b < whole; b += 512) {
            const uint64_t v = ld64u(src + b);
            __builtin_memcpy(dst + b, &v, 8);
        }
        if (whole + lane < n) dst[whole + lane] = src[whole + lane];
    }
    if (bad && lane == 0) __hip_atomic_fetch_or(&a.ctrl[kTakeCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oxh

namespace {

using oxh::cols::is_bytes;
namespace take = oxh::take;

// oxh_set_kernel_variant(kVariantTake + 8 * p + t): the threshold kTakeThresholds[t] and the piece size
// kTakePieces[p] instead of the shipped pair (tools/take_probe.py)
constexpr int kVariantTake = 9100;
constexpr uint32_t kTakeThresholds[8] = {0, 32, 64, 128, 256, 512, 1024, 4096};
constexpr uint32_t kTakePieces[8] = {256, 512, 1024, 2048, 4096, 8192, 16384, 65536};

unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }
uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

int take_error(unsigned long long e) {
    if (!e) return OXH_OK;
    if (e & oxh::kTakeErrPlace) return fail(OXH_ERR_HIP, "take: the cells changed between the passes of one call");
    if (e & oxh::kTakeErrIndex) return fail(OXH_ERR_INVALID, "take: an index is neither OXH_TAKE_NULL nor below its column's rows");
    if (e & oxh::kRowErrOffsets) return fail(OXH_ERR_INVALID, "take: a byte column's offsets decrease or are negative");
    if (e & oxh::kTakeErrLength) return fail(OXH_ERR_INVALID, "take: a cell is longer than 2^32 - 1 bytes");
    return fail(OXH_ERR_INVALID, "take: a byte column has bytes but no values");
}

// One call over device-resident sources and indices. The small block holds [TakeSrc nsrc | TakeOut nout |
// ctrl | one total per output column], on the device and pinned; the byte columns' lengths, offsets and scan
// sums are leased from scratch.hpp for the call; the item lists of the long cells get a block of their own,
// since their number is known only after the measure pass.
struct TakeCall {
    const take::Args& a;
    hipStream_t st;
    CallBlock block;
    std::unique_ptr<oxh::ScratchLease> lease;  // ends (and waits for the stream) before the block is freed
    uint8_t* d_lists = nullptr;
    size_t out_at = 0, ctrl_at = 0, totals_at = 0, bytes = 0;
    std::vector<uint32_t> byte_cols;
    std::vector<uint64_t> need;  // value bytes of every output column
    uint64_t nlong = 0, npieces = 0;
    oxh::TakeArgs k{};

    TakeCall(const take::Args& args, hipStream_t stream) : a(args), st(stream), need(args.nout, 0) {}
    ~TakeCall() {
        if (d_lists) {
            (void)hipStreamSynchronize(st);
            (void)hipFree(d_lists);
        }
    }

    oxh::TakeOut* h_out() { return (oxh::TakeOut*)(block.h + out_at); }
    const unsigned long long* h_ctrl() { return (const unsigned long long*)(block.h + ctrl_at); }

    int make(const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bits,
             const uint32_t* d_idx0, const uint32_t* d_idx1) {
        const int variant = g_variant.load();
        const bool probe = variant >= kVariantTake && variant < kVariantTake + 64;
        k.short_max = probe ? kTakeThresholds[(variant - kVariantTake) & 7] : oxh::kTakeShortMax;
        k.piece = probe ? kTakePieces[(variant - kVariantTake) >> 3] : oxh::kTakePiece;
        out_at = (a.nsrc * sizeof(oxh::TakeSrc) + 63) & ~(size_t)63;
        ctrl_at = (out_at + a.nout * sizeof(oxh::TakeOut) + 63) & ~(size_t)63;
        totals_at = ctrl_at + oxh::kTakeCtrlWords * 8;
        bytes = totals_at + a.nout * 8;
        int rc = block.make(bytes, "take", st);
        if (rc) return rc;
        oxh::TakeSrc* src = (oxh::TakeSrc*)block.h;
        for (uint32_t c = 0; c < a.nsrc; ++c) {
            src[c].col.values = (const uint8_t*)d_values[c];
            src[c].col.offsets = is_bytes(a.kinds[c]) ? (const uint8_t*)d_offsets[c] : nullptr;
            src[c].col.validity = d_validity[c];
            src[c].col.vbit = bits[2 * c];
            src[c].col.nbit = bits[2 * c + 1];
            src[c].col.kind = a.kinds[c];
            src[c].rows = a.src_rows[c];
        }
        for (uint32_t o = 0; o < a.nout; ++o) {
            const uint32_t* p = a.plan + 4 * o;
            oxh::TakeOut& out = h_out()[o];
            out.a = p[0], out.ia = p[1], out.b = p[2], out.ib = p[3];
            out.kind = a.kinds[p[0]];
            if (is_bytes(out.kind)) byte_cols.push_back(o);
            else need[o] = take::plain_value_bytes(out.kind, a.nout_rows);
        }
        k.src = (const oxh::TakeSrc*)block.d;
        k.out = (const oxh::TakeOut*)(block.d + out_at);
        k.idx0 = d_idx0, k.idx1 = d_idx1;
        k.n = a.nout_rows, k.nout = a.nout;
        k.ctrl = (unsigned long long*)(block.d + ctrl_at);
        if (byte_cols.empty()) return OXH_OK;
        // per byte column: [len n u32 | off n u64 | scan sums tiles + 1 u64], each 256-B aligned
        const uint64_t n = a.nout_rows, tiles = oxh::scan_tiles(n);
        const uint64_t len_bytes = align256(n * 4), off_bytes = align256(n * 8), per = len_bytes + off_bytes + align256((tiles + 1) * 8);
        lease.reset(new oxh::ScratchLease(st));
        void* base = nullptr;
        if (lease->get(per * byte_cols.size(), &base) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "take: " + std::to_string(per * byte_cols.size()) + " B of lengths and offsets");
        }
        for (size_t j = 0; j < byte_cols.size(); ++j) {
            oxh::TakeOut& out = h_out()[byte_cols[j]];
            uint8_t* at = (uint8_t*)base + j * per;
            out.len = (uint32_t*)at;
            out.off = (const uint64_t*)(at + len_bytes);
            out.total = (const unsigned long long*)(at + len_bytes + off_bytes) + tiles;
        }
        return OXH_OK;
    }

    int read_ctrl() {
        HIP_TRY(hipMemcpyAsync(block.h + ctrl_at, block.d + ctrl_at, oxh::kTakeCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return take_error(h_ctrl()[oxh::kTakeCtrlErr]);
    }

    // need[] of every column; complete on return. Without byte columns the host knows the sizes already.
    int measure() {
        if (byte_cols.empty()) return OXH_OK;
        HIP_TRY(hipMemcpyAsync(block.d, block.h, totals_at, hipMemcpyHostToDevice, st));  // the ctrl words are 0
        oxh::take_resolve_kernel<false><<<grid_for(k.n), 256, 0, st>>>(k);
        HIP_TRY(hipGetLastError());
        unsigned long long* h_totals = (unsigned long long*)(block.h + totals_at);
        for (uint32_t o : byte_cols) {
            const oxh::TakeOut& out = h_out()[o];
            const uint64_t tiles = oxh::scan_tiles(k.n);
            int rc = oxh::exclusive_scan_u32(out.len, k.n, const_cast<uint64_t*>(out.off),
                                             const_cast<unsigned long long*>(out.total) - tiles, st);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(&h_totals[o], out.total, 8, hipMemcpyDeviceToHost, st));
        }
        int rc = read_ctrl();  // the call's one round trip before the outputs
        if (rc) return rc;
        nlong = h_ctrl()[oxh::kTakeCtrlLong], npieces = h_ctrl()[oxh::kTakeCtrlPieces];
        for (uint32_t o : byte_cols) {
            need[o] = h_totals[o];
            if (h_out()[o].kind == OXH_COL_BYTES32 && need[o] > take::kMaxBytes32)
                return fail(OXH_ERR_INVALID, "take: output column " + std::to_string(o) + " holds " + std::to_string(need[o]) +
                                                 " B, more than int32 offsets can say: pass the column as OXH_COL_BYTES64");
        }
        STEP("take: %llu rows, %zu byte columns, %llu long cells in %llu pieces", (unsigned long long)k.n, byte_cols.size(),
             (unsigned long long)nlong, (unsigned long long)npieces);
        return OXH_OK;
    }

    bool fits() const {
        for (uint32_t o : byte_cols)
            if (need[o] > a.value_capacity[o]) return false;
        return true;
    }

    // Every output, to device buffers; complete on return.
    int write(void* const* d_out_values, void* const* d_out_offsets, uint8_t* const* d_out_validity) {
        for (uint32_t o = 0; o < a.nout; ++o) {
            oxh::TakeOut& out = h_out()[o];
            out.values = (uint8_t*)d_out_values[o];
            out.offsets = (uint8_t*)d_out_offsets[o];
            out.validity = d_out_validity[o];
        }
        HIP_TRY(hipMemcpyAsync(block.d, block.h, ctrl_at, hipMemcpyHostToDevice, st));
        if (byte_cols.empty()) HIP_TRY(hipMemsetAsync(k.ctrl, 0, oxh::kTakeCtrlWords * 8, st));
        oxh::take_resolve_kernel<true><<<grid_for(k.n), 256, 0, st>>>(k);
        HIP_TRY(hipGetLastError());
        if (npieces) {
            // [item_cp npieces u64 | item_row npieces u32], 0xFF-filled
            if (hipMalloc(&d_lists, npieces * 12) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(st);
                return fail(OXH_ERR_NOMEM, "take: the lists of " + std::to_string(npieces) + " pieces of long cells");
            }
            oxh::poison_device(d_lists, npieces * 12, st);
            k.item_cp = (uint64_t*)d_lists;
            k.item_row = (uint32_t*)(d_lists + npieces * 8);
            k.nitems = npieces;
            HIP_TRY(hipMemsetAsync(d_lists, 0xFF, npieces * 12, st));
            oxh::take_long_plan_kernel<<<grid_for(k.n), 256, 0, st>>>(k);
            HIP_TRY(hipGetLastError());
            oxh::take_long_gather_kernel<<<(unsigned)((npieces + 3) / 4), 256, 0, st>>>(k);
            HIP_TRY(hipGetLastError());
        }
        int rc = read_ctrl();
        if (rc == OXH_OK && h_ctrl()[oxh::kTakeCtrlCursor] != npieces)  // fewer pieces listed than counted
            rc = take_error(oxh::kTakeErrPlace);
        return rc;
    }
};

// What both forms do before they need a device. `done`: no output rows, nothing left to do.
int take_enter(oxh_ctx* ctx, const take::Args& a, bool host, bool& done) {
    done = false;
    const std::string what = take::argument_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "take: " + what);
    if (a.nout_rows == 0) {
        bool offsets = false;  // a byte column's single 0 is device memory in the device form
        for (uint32_t o = 0; o < a.nout && !take::sizes_only(a); ++o) {
            const uint32_t kind = take::out_kind(a, o);
            if (!is_bytes(kind)) continue;
            if (host) memset(a.out_offsets[o], 0, oxh::cols::offset_width(kind));
            offsets = true;
        }
        if (host || !offsets) {
            memset(a.value_bytes, 0, a.nout * sizeof(uint64_t));
            *a.written = take::sizes_only(a) ? 0 : 1;
            done = true;
            return OXH_OK;
        }
    }
    return device_enter(ctx);
}

}  // namespace

extern "C" {

int oxh_take_columns_device(oxh_ctx* ctx, uint32_t nsrc, const uint32_t* kinds, const void* const* d_values,
                            const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                            const uint64_t* src_rows, uint64_t nout_rows, const uint32_t* d_idx0, const uint32_t* d_idx1,
                            uint32_t nout, const uint32_t* plan, const uint64_t* value_capacity, void* const* d_out_values,
                            void* const* d_out_offsets, uint8_t* const* d_out_validity, uint64_t* value_bytes, uint32_t* written,
                            void* stream) {
    const take::Args a{nsrc, kinds, d_values, d_offsets, d_validity, bit_offsets, src_rows, nout_rows, d_idx0, d_idx1, nout, plan,
                       value_capacity, d_out_values, d_out_offsets, d_out_validity, value_bytes, written};
    bool done = false;
    int rc = take_enter(ctx, a, false, done);
    if (rc || done) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (nout_rows == 0) {  // outputs given: the byte columns' single offset
        for (uint32_t o = 0; o < nout; ++o)
            if (is_bytes(take::out_kind(a, o)))
                HIP_TRY(hipMemsetAsync(d_out_offsets[o], 0, oxh::cols::offset_width(take::out_kind(a, o)), st));
        HIP_TRY(hipStreamSynchronize(st));
        memset(value_bytes, 0, nout * sizeof(uint64_t));
        *written = 1;
        return OXH_OK;
    }
    TakeCall call(a, st);
    if ((rc = call.make(d_values, d_offsets, d_validity, bit_offsets, d_idx0, d_idx1))) return rc;
    if ((rc = call.measure())) return rc;
    const bool fits = !take::sizes_only(a) && call.fits();
    if (fits && (rc = call.write(d_out_values, d_out_offsets, d_out_validity))) return rc;
    memcpy(value_bytes, call.need.data(), nout * sizeof(uint64_t));
    *written = fits ? 1 : 0;
    return OXH_OK;
}

int oxh_take_columns_host(oxh_ctx* ctx, uint32_t nsrc, const uint32_t* kinds, const void* const* values,
                          const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                          const uint64_t* src_rows, uint64_t nout_rows, const uint32_t* idx0, const uint32_t* idx1, uint32_t nout,
                          const uint32_t* plan, const uint64_t* value_capacity, void* const* out_values, void* const* out_offsets,
                          uint8_t* const* out_validity, uint64_t* value_bytes, uint32_t* written) {
    const take::Args a{nsrc, kinds, values, offsets, validity, bit_offsets, src_rows, nout_rows, idx0, idx1, nout, plan,
                       value_capacity, out_values, out_offsets, out_validity, value_bytes, written};
    bool done = false;
    int rc = take_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // One device block for the inputs: for every source column only what its rows name (columns.hpp), then
    // the index arrays. The outputs get a block of their own once their sizes are known.
    oxh::cols::Staging plan_in;
    std::vector<oxh::cols::Staged> staged(nsrc);
    for (uint32_t c = 0; c < nsrc; ++c)
        if (src_rows[c])
            staged[c] = plan_in.add_column(kinds[c], values[c], offsets[c], validity[c], bit_offsets[2 * c], bit_offsets[2 * c + 1],
                                           src_rows[c]);
    const int64_t at0 = idx0 ? plan_in.add(idx0, nout_rows * 4) : -1, at1 = idx1 ? plan_in.add(idx1, nout_rows * 4) : -1;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_in, plan_in.total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "take: " + std::to_string(plan_in.total) + " B for the columns on the device");
    }
    oxh::poison_device(d_in, plan_in.total + 16, st);
    std::vector<uint64_t> need;
    bool fits = false;
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : plan_in.pieces)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(d_in + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        std::vector<const void*> d_values(nsrc), d_offsets(nsrc);
        std::vector<const uint8_t*> d_validity(nsrc);
        std::vector<uint64_t> bits(2 * (size_t)nsrc, 0);
        for (uint32_t c = 0; c < nsrc; ++c) {
            d_values[c] = plan_in.values_at(d_in, staged[c]);
            d_offsets[c] = plan_in.offsets_at(d_in, staged[c]);
            d_validity[c] = plan_in.validity_at(d_in, staged[c]);
            bits[2 * c] = staged[c].vbit, bits[2 * c + 1] = staged[c].nbit;
        }
        auto idx_at = [&](int64_t piece) { return piece < 0 ? nullptr : (const uint32_t*)(d_in + plan_in.pieces[piece].at); };
        TakeCall call(a, st);
        int r = call.make(d_values.data(), d_offsets.data(), d_validity.data(), bits.data(), idx_at(at0), idx_at(at1));
        if (r || (r = call.measure())) return r;
        need = call.need;
        fits = !take::sizes_only(a) && call.fits();
        if (!fits) return OXH_OK;
        const take::OutBlock where(a, need.data());
        if (hipMalloc(&d_out, where.total + 16) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "take: " + std::to_string(where.total) + " B for the output columns on the device");
        }
        oxh::poison_device(d_out, where.total + 16, st);
        std::vector<void*> o_values(nout), o_offsets(nout);
        std::vector<uint8_t*> o_validity(nout);
        for (uint32_t o = 0; o < nout; ++o) {
            o_validity[o] = d_out + where.at[3 * o];
            o_values[o] = d_out + where.at[3 * o + 1];
            o_offsets[o] = d_out + where.at[3 * o + 2];
        }
        if ((r = call.write(o_values.data(), o_offsets.data(), o_validity.data()))) return r;
        for (uint32_t o = 0; o < nout; ++o) {
            const uint32_t kind = take::out_kind(a, o);
            HIP_TRY(hipMemcpyAsync(out_validity[o], o_validity[o], take::bitmap_bytes(nout_rows), hipMemcpyDeviceToHost, st));
            if (need[o]) HIP_TRY(hipMemcpyAsync(out_values[o], o_values[o], need[o], hipMemcpyDeviceToHost, st));
            if (is_bytes(kind))
                HIP_TRY(hipMemcpyAsync(out_offsets[o], o_offsets[o], (nout_rows + 1) * oxh::cols::offset_width(kind),
                                       hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (rc) return rc;
    memcpy(value_bytes, need.data(), nout * sizeof(uint64_t));
    *written = fits ? 1 : 0;
    return OXH_OK;
}

}  // extern "C"
