// oxen_amd/csrc/json_write.hip -- typed Arrow columns in HBM to the bytes of a JSON Lines or JSON file
// (oxh_write_json_*): `write_df`'s jsonl / ndjson / json arms (core/df/tabular.rs:1469-1490, 1536-1538) and the text of
// every data-frame view the server returns (view/json_data_frame_view.rs:268-285). The rules are stated in
// include/oxen_hash.h "JSON text" (DESIGN.md §4 "JSON text"); a value's text is json_text.hpp's (and through it
// csv_text.hpp's), the code tests/native/json_write_host_test.cpp runs on the host. The CSV writer's passes
// (csv_write.hip) with every row carrying its keys -- lengths, scan, emit -- on one stream:
//   keys     the host builds, per column, the constant bytes in front of its value ({"a": for column 0, ,"b": for the
//            others); they sit in the call's small block. A row's closing '}' is followed by one byte: '\n', or ','
//            and for the last row ']' in the array form, so both formats share every length;
//   length   jsonw_length_kernel: one lane per row walks all the columns of its row: the row's text length (u32), its
//            count of deferred float cells, and the stats. A string cell of kLongCell bytes and more is counted by
//            the whole wave, 8 bytes a lane and step;
//   deferral (only when a float cell was deferred) exclusive_scan_u32 over the rows' counts gives each row its first
//            slot; jsonw_defer_list_kernel writes the cells' bits in (row, column) order; they come down, the host
//            formats them (csv_text.hpp's deferred_slot) into 32-byte slots that go up again, and
//            jsonw_defer_add_kernel adds their lengths to their rows;
//   scan     exclusive_scan_u32 over the lengths: the u64 start of every row, and the total;
//   emit     jsonw_emit_kernel: the 64 rows of a wave own one contiguous span of the output. Its rows below kLongCell
//            bytes are assembled in the wave's own LDS, at the destination's own misalignment, and stored 16 bytes
//            a lane on the destination's 16-byte grid: the whole span at once when it fits kJsonwSpanLds bytes, else
//            in runs of neighbouring rows that do. A row of kLongCell bytes and more is written by its lane straight
//            to the output, and a string cell of kLongCell source bytes and more by the whole wave: copy_span_wave
//            where no byte widens, else 512 source bytes a step (8 a lane in one load), a lane's place the wave
//            prefix sum of the widths (1, 2 or 6) in front of its bytes; the widened text is staged in the wave's
//            LDS and stored in aligned 16-byte blocks (measured against 64 source bytes a step stored byte by byte:
//            DESIGN.md §4 "JSON text").
// No workgroup waits for another; launches order the steps. Every store is checked against the row's own span
// first: columns that change during the call set the error word (OXH_ERR_HIP), they do not write outside.
// The host-side call (arguments, lease, deferral) restates csv_write.hip's; DESIGN.md §7 names the follow-up.
// Needs IEEE division and no fast-math (csv_text.hpp's exact path).
#include "capi_internal.hpp"
#include "columns.hpp"
#include "json_text.hpp"

using namespace oxh::capi;

namespace oxh {

__constant__ double kJsonwPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                       1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

constexpr uint32_t kJsonwLongCell = csvtext::kLongCell;
constexpr uint32_t kJsonwDeferSlot = csvtext::kDeferSlot;
constexpr uint32_t kJsonwSpanLds = 8192;     // the most bytes of a wave's span that is assembled in LDS
constexpr unsigned kJsonwMaxGroups = 2048;   // workgroups of a row-per-lane launch; the rest by grid stride
constexpr uint64_t kJsonwMaxRowText = 1ull << 32;
constexpr unsigned long long kJsonwErrRowText = 4, kJsonwErrPlace = 8;  // beside kRowErrOffsets, kRowErrValues
// ctrl words: the error word, the escaped string cells, the cells written as null, the deferred cells
constexpr int kJsonwErr = 0, kJsonwEscaped = 1, kJsonwNulls = 2, kJsonwDeferred = 3, kJsonwCtrlWords = 8;

struct JsonwCol {
    RowCol c;
    const uint8_t* key;  // the bytes in front of the column's value, in the call's small block
    uint32_t type;       // OXH_CSV_*
    uint32_t key_len;
};

struct JsonwArgs {
    const JsonwCol* cols;
    uint64_t nrows;
    uint64_t key_bytes;      // of all columns together
    uint32_t ncols;
    uint32_t term, last_term;  // the byte behind a row's '}', and behind the last row's
};

__device__ __forceinline__ bool jsonw_is_string(uint32_t type) { return type == OXH_CSV_STRING || type == OXH_CSV_STRING64; }
__device__ __forceinline__ bool jsonw_present(const RowCol& c, uint64_t r) { return !c.validity || row_bit(c.validity, c.nbit + r); }

__device__ __forceinline__ unsigned long long jsonw_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
    return v;
}

// The escaped length of the n bytes at p, by a whole wave (every lane calls it with the same arguments): 8 bytes a
// lane and step, the last n % 8 bytes one lane each.
__device__ __forceinline__ uint64_t jsonw_wave_count(const uint8_t* p, uint64_t n, unsigned lane) {
    unsigned long long mine = 0;
    const uint64_t whole = n & ~7ull;
    for (uint64_t b = 8ull * lane; b < whole; b += 512) {
        const uint64_t w = ld64u(p + b);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) mine += jsontext::byte_width((uint32_t)(w >> (8 * k)) & 0xFF);
    }
    if (whole + lane < n) mine += jsontext::byte_width(p[whole + lane]);
    return jsonw_wave_sum(mine);
}

typedef uint32_t JsonwBlock16 __attribute__((ext_vector_type(4)));  // one 16-byte block
// The output is global memory; saying so keeps the stores off the flat path.
#define OXH_JSONW_GLOBAL __attribute__((address_space(1)))

// The LDS of the emit kernel is private to a wave: its lanes write their bytes, then all 64 read the span. A wave's
// LDS operations execute in order, so nothing has to be waited for; the fences only keep the compiler from moving
// them across (they emit no instruction).
__device__ __forceinline__ void jsonw_wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr uint32_t kJsonwEscapeStep = 512;                       // source bytes of one step: 8 a lane
constexpr uint32_t kJsonwEscapeMost = 6 * kJsonwEscapeStep;      // the most bytes one step adds

// The n bytes at p escaped to dst[0 .. room), by a whole wave through its own LDS (`stage`, kJsonwSpanLds + 16 bytes,
// free while the wave writes its long rows): 512 source bytes a step, 8 a lane in one load; a lane's place is the
// wave prefix sum of the widths in front of its 8 bytes. The text is staged at the destination's misalignment and
// stored 16 bytes a lane on the destination's grid whenever another step might not fit; the bytes behind the last
// whole block move to the front and wait for the next store. No byte is stored at or behind dst + room.
__device__ __forceinline__ void jsonw_wave_escape(uint8_t* dst, uint64_t room, const uint8_t* p, uint64_t n, unsigned lane, uint8_t* stage) {
    static_assert(kJsonwEscapeMost + 16 <= kJsonwSpanLds, "a step fits the stage behind a kept tail");
    const uintptr_t end = (uintptr_t)dst + room;
    uintptr_t grid = (uintptr_t)dst & ~(uintptr_t)15;  // where stage[0] goes
    uint32_t lo = (uint32_t)((uintptr_t)dst & 15);     // stage[lo .. fill) waits to be stored
    uint32_t fill = lo;
    for (uint64_t at = 0; at < n; at += kJsonwEscapeStep) {
        const uint64_t mine = at + 8ull * lane;
        const uint32_t have = mine >= n ? 0u : n - mine < 8 ? (uint32_t)(n - mine) : 8u;
        uint64_t word = 0;
        if (have == 8) {
            word = ld64u(p + mine);
        } else {
            for (uint32_t k = 0; k < have; ++k) word |= (uint64_t)p[mine + k] << (8 * k);
        }
        uint32_t w = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            if (k < have) w += jsontext::byte_width((uint32_t)(word >> (8 * k)) & 0xFF);
        uint32_t incl = w;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t below = (uint32_t)__shfl_up((int)incl, off, 64);
            if ((int)lane >= off) incl += below;
        }
        uint32_t o = fill + incl - w;  // + w <= fill + kJsonwEscapeMost <= kJsonwSpanLds + 16
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            if (k < have) o += jsontext::byte_put((uint32_t)(word >> (8 * k)) & 0xFF, stage + o);
        fill += (uint32_t)__shfl((int)incl, 63, 64);
        const bool last = at + kJsonwEscapeStep >= n;
        if (!last && fill + kJsonwEscapeMost <= kJsonwSpanLds + 16) continue;  // uniform
        jsonw_wave_lds_order();  // the steps are staged
        const uint32_t upto = last ? fill : fill & ~15u;
        for (uint32_t b = 16 * lane; b < upto; b += 16 * 64) {
            const uintptr_t to = grid + b;
            if (b >= lo && b + 16 <= upto && to + 16 <= end) {
                *(OXH_JSONW_GLOBAL JsonwBlock16*)to = *(const JsonwBlock16*)&stage[b];
            } else {  // the block holds the text's head or tail: only the bytes inside
                for (uint32_t k = 0; k < 16; ++k)
                    if (b + k >= lo && b + k < upto && to + k < end) *(OXH_JSONW_GLOBAL uint8_t*)(to + k) = stage[b + k];
            }
        }
        const uint32_t rest = fill - upto;  // < 16, and 0 after the last step
        const uint8_t kept = lane < rest ? stage[upto + lane] : (uint8_t)0;
        jsonw_wave_lds_order();  // the blocks are stored, the tail is read
        if (lane < rest) stage[lane] = kept;
        jsonw_wave_lds_order();
        grid += upto, fill = rest, lo = 0;
    }
}

// ---------------------------------------------------------------- lengths
__global__ __launch_bounds__(256) void jsonw_length_kernel(const JsonwArgs a, uint32_t* __restrict__ lens, uint32_t* __restrict__ defer_counts,
                                                           unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = a.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: the long cells are a whole wave's
    unsigned long long bad = 0, n_escaped = 0, n_null = 0, n_deferred = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        const bool live = i < n;
        uint64_t len = live ? a.key_bytes + 2 : 0;  // the keys, '}' and the byte behind it
        uint32_t ndef = 0;
        for (uint32_t c = 0; c < a.ncols; ++c) {
            const JsonwCol& wc = a.cols[c];
            uint64_t start = 0, cell = 0;
            bool is_long = false;
            if (live) {
                if (!jsonw_present(wc.c, i)) {
                    ++n_null;
                    len += jsontext::kNullText;
                } else if (wc.type == OXH_CSV_INT64) {
                    len += csvtext::int64_text((int64_t)ld64u(wc.c.values + 8 * i), nullptr);
                } else if (wc.type == OXH_CSV_BOOL) {
                    len += csvtext::bool_text(row_bit(wc.c.values, wc.c.vbit + i), nullptr);
                } else if (wc.type == OXH_CSV_FLOAT64) {
                    const csvtext::FloatForm f = csvtext::float_form(ld64u(wc.c.values + 8 * i), kJsonwPow10);
                    if (f.kind == csvtext::kFormDeferred) {
                        ++ndef;
                    } else {
                        n_null += f.kind == csvtext::kFormNan || f.kind == csvtext::kFormInf;
                        len += jsontext::float_form_text(f, nullptr);
                    }
                } else {
                    cell = row_cell(wc.c, i, start, bad);
                    is_long = cell >= kJsonwLongCell;
                    if (!is_long) {
                        const uint64_t l = jsontext::escaped_len(wc.c.values + start, cell);
                        len += l + 2;
                        n_escaped += l != cell;
                    }
                }
            }
            if (!jsonw_is_string(wc.type)) continue;  // uniform
            unsigned long long todo = __ballot(is_long);
            while (todo) {  // uniform in the wave
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1;
                const uint64_t from = (uint64_t)__shfl((long long)start, src, 64), count = (uint64_t)__shfl((long long)cell, src, 64);
                const uint64_t l = jsonw_wave_count(wc.c.values + from, count, lane);
                if ((int)lane == src) {
                    len += l + 2;
                    n_escaped += l != count;
                }
            }
        }
        if (live) {
            if (len >= kJsonwMaxRowText) bad |= kJsonwErrRowText, len = 0;
            lens[i] = (uint32_t)len;
            if (defer_counts) defer_counts[i] = ndef;
            n_deferred += ndef;
        }
    }
    n_escaped = jsonw_wave_sum(n_escaped), n_null = jsonw_wave_sum(n_null), n_deferred = jsonw_wave_sum(n_deferred);
    if (lane == 0) {
        if (n_escaped) atomicAdd(&ctrl[kJsonwEscaped], n_escaped);
        if (n_null) atomicAdd(&ctrl[kJsonwNulls], n_null);
        if (n_deferred) atomicAdd(&ctrl[kJsonwDeferred], n_deferred);
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJsonwErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- the deferred floats
// (the counts are scanned into `first`) list[first[i] + j] = the bits of row i's j-th deferred cell, in column order.
__global__ __launch_bounds__(256) void jsonw_defer_list_kernel(const JsonwArgs a, const uint32_t* __restrict__ counts,
                                                               const uint64_t* __restrict__ first, uint64_t ndeferred,
                                                               uint64_t* __restrict__ list, unsigned long long* __restrict__ ctrl) {
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nrows; i += stride) {
        if (!counts[i]) continue;
        uint64_t slot = first[i];
        const uint64_t end = slot + counts[i];
        for (uint32_t c = 0; c < a.ncols; ++c) {
            const JsonwCol& wc = a.cols[c];
            if (wc.type != OXH_CSV_FLOAT64 || !jsonw_present(wc.c, i)) continue;
            const uint64_t bits = ld64u(wc.c.values + 8 * i);
            if (csvtext::float_form(bits, kJsonwPow10).kind != csvtext::kFormDeferred) continue;
            if (slot >= end || slot >= ndeferred) {
                bad |= kJsonwErrPlace;
                break;
            }
            list[slot++] = bits;
        }
        if (slot != end) bad |= kJsonwErrPlace;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJsonwErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (the slots hold the host's texts) lens[i] += the lengths of row i's deferred cells.
__global__ __launch_bounds__(256) void jsonw_defer_add_kernel(const uint32_t* __restrict__ counts, const uint64_t* __restrict__ first, uint64_t nrows,
                                                              const uint8_t* __restrict__ slots, uint64_t ndeferred, uint32_t* __restrict__ lens,
                                                              unsigned long long* __restrict__ ctrl) {
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += stride) {
        const uint32_t cnt = counts[i];
        if (!cnt) continue;
        const uint64_t at = first[i];
        if (at + cnt > ndeferred) {
            bad |= kJsonwErrPlace;
            continue;
        }
        uint64_t len = lens[i];
        for (uint32_t j = 0; j < cnt; ++j) len += slots[(at + j) * kJsonwDeferSlot + kJsonwDeferSlot - 1];
        if (len >= kJsonwMaxRowText) bad |= kJsonwErrRowText, len = 0;
        lens[i] = (uint32_t)len;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJsonwErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- emit
struct JsonwEmit {
    const uint32_t* lens;
    const uint64_t* starts;
    const uint64_t* defer_first;  // NULL: no cell was deferred
    const uint8_t* slots;
    uint64_t ndeferred;
    uint64_t total;               // the rows' bytes
    uint8_t* out;                 // where row 0 starts
};

// n bytes to dst by one lane: into LDS byte by byte, to the output the widest pieces first.
template <bool LDS>
__device__ __forceinline__ void jsonw_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    if constexpr (LDS) {
        for (uint32_t b = 0; b < n; ++b) dst[b] = src[b];
    } else {
        copy_span_lane(dst, src, n);
    }
}

// Row i's text to dst[0 .. len), by its lane. LDS false: every lane of the wave calls it (live or not) and a string
// cell of kJsonwLongCell bytes and more is written by the whole wave; LDS true: such a cell cannot be in a row that
// is assembled here (the row alone would be longer) and counts as a changed column. stage: the wave's LDS, for the
// long cells that widen (LDS false only).
template <bool LDS>
__device__ __forceinline__ void jsonw_emit_row(const JsonwArgs& a, const JsonwEmit& e, uint8_t* dst, bool live, uint64_t i, uint32_t len,
                                               unsigned lane, uint8_t* stage, unsigned long long& bad) {
    uint64_t o = 0;  // the bytes of the row so far; > len: the row has failed, nothing more is stored
    uint64_t slot = live && e.defer_first ? e.defer_first[i] : 0;
    for (uint32_t c = 0; c < a.ncols; ++c) {
        const JsonwCol& wc = a.cols[c];
        uint64_t start = 0, cell = 0;
        bool is_long = false;
        if (live && o <= len) {
            if (o + wc.key_len <= len) jsonw_copy<LDS>(dst + o, wc.key, wc.key_len);
            o += wc.key_len;
            if (!jsonw_present(wc.c, i)) {
                if (o + jsontext::kNullText <= len) jsontext::null_put(dst + o);
                o += jsontext::kNullText;
            } else if (wc.type == OXH_CSV_INT64) {
                const int64_t v = (int64_t)ld64u(wc.c.values + 8 * i);
                const uint32_t l = csvtext::int64_text(v, nullptr);
                if (o + l <= len) csvtext::int64_text(v, dst + o);
                o += l;
            } else if (wc.type == OXH_CSV_BOOL) {
                const bool v = row_bit(wc.c.values, wc.c.vbit + i);
                const uint32_t l = csvtext::bool_text(v, nullptr);
                if (o + l <= len) csvtext::bool_text(v, dst + o);
                o += l;
            } else if (wc.type == OXH_CSV_FLOAT64) {
                const csvtext::FloatForm f = csvtext::float_form(ld64u(wc.c.values + 8 * i), kJsonwPow10);
                if (f.kind != csvtext::kFormDeferred) {
                    const uint32_t l = jsontext::float_form_text(f, nullptr);
                    if (o + l <= len) jsontext::float_form_text(f, dst + o);
                    o += l;
                } else if (slot < e.ndeferred) {
                    const uint8_t* text = e.slots + slot * kJsonwDeferSlot;
                    const uint32_t l = text[kJsonwDeferSlot - 1];
                    if (l <= csvtext::kMaxFloatText && o + l <= len) {
                        for (uint32_t b = 0; b < l; ++b) dst[o + b] = text[b];
                        o += l;
                    } else {
                        o = (uint64_t)len + 1;
                    }
                    ++slot;
                } else {
                    o = (uint64_t)len + 1;
                }
            } else {
                cell = row_cell(wc.c, i, start, bad);
                is_long = cell >= kJsonwLongCell;
                if (!is_long) {
                    const uint64_t l = jsontext::escaped_len(wc.c.values + start, cell) + 2;
                    if (o + l <= len) {
                        if (l != cell + 2) {
                            if (jsontext::string_put(wc.c.values + start, cell, dst + o, l) != l) o = (uint64_t)len + 1;  // the cell changed
                        } else {
                            dst[o] = '"';
                            jsonw_copy<LDS>(dst + o + 1, wc.c.values + start, (uint32_t)cell);
                            dst[o + l - 1] = '"';
                        }
                    }
                    o += l;
                } else if (LDS) {
                    o = (uint64_t)len + 1;
                }
            }
        }
        if constexpr (!LDS) {
            if (!jsonw_is_string(wc.type)) continue;  // uniform
            unsigned long long todo = __ballot(is_long);
            while (todo) {  // uniform in the wave
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1;
                const uint8_t* p = wc.c.values + (uint64_t)__shfl((long long)start, src, 64);
                const uint64_t count = (uint64_t)__shfl((long long)cell, src, 64);
                const uint64_t at = (uint64_t)__shfl((long long)o, src, 64), room = (uint64_t)__shfl((long long)(uint64_t)len, src, 64);
                uint8_t* d = (uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)dst, src, 64) + at;
                const uint64_t inner = jsonw_wave_count(p, count, lane), l = inner + 2;
                if (at <= room && at + l <= room) {
                    if (lane == 0) d[0] = '"', d[l - 1] = '"';
                    if (inner == count)
                        copy_span_wave(d + 1, p, count, lane);
                    else
                        jsonw_wave_escape(d + 1, inner, p, count, lane, stage);
                }
                if ((int)lane == src) o += l;
            }
        }
    }
    if (live) {
        if (o + 2 == len)
            dst[o] = '}', dst[o + 1] = (uint8_t)(i + 1 == a.nrows ? a.last_term : a.term);
        else
            bad |= kJsonwErrPlace;  // the row's text is not what the length pass measured
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void jsonw_emit_kernel(const JsonwArgs a, const JsonwEmit e, unsigned long long* __restrict__ ctrl) {
    __shared__ __attribute__((aligned(16))) uint8_t spans[4][kJsonwSpanLds + 16];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n = a.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform in the wave: the runs, the long cells
    unsigned long long bad = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool live = i < n;
        uint64_t at = 0;
        uint32_t len = 0;
        if (live) {
            at = e.starts[i], len = e.lens[i];
            if (at + len > e.total || len == 0) bad |= kJsonwErrPlace, live = false, len = 0;  // never a store outside the total bytes
        }
        // 1. The rows below kJsonwLongCell bytes, run by run through LDS. A run is the neighbouring rows, from the
        // first one not yet written on, whose span still fits: a wave of short rows is one run, a wave of 370-byte
        // rows three. A longer row or a dead lane ends a run (the output would not be contiguous across it).
        const bool short_row = live && len < kJsonwLongCell;
        unsigned long long todo = __ballot(short_row);
        while (todo) {  // uniform in the wave
            const int first = __builtin_ctzll(todo);
            const uint64_t lo = (uint64_t)__shfl((long long)at, first, 64);
            const bool fits = short_row && (int)lane >= first && at >= lo && at + len - lo <= kJsonwSpanLds;  // lane `first` always does
            const unsigned long long gaps = ~__ballot(fits) & (~0ull << first);
            const int stop = gaps ? __builtin_ctzll(gaps) : 64;                       // the first lane behind the run
            const unsigned long long run = (stop == 64 ? ~0ull : (1ull << stop) - 1) & (~0ull << first);
            const bool mine = (run >> lane) & 1;
            const uint64_t hi = (uint64_t)__shfl((long long)(at + len), stop - 1, 64);
            const uint32_t shift = (uint32_t)((uintptr_t)(e.out + lo) & 15);
            jsonw_emit_row<true>(a, e, &spans[wave][shift + (mine ? (uint32_t)(at - lo) : 0u)], mine, i, len, lane, nullptr, bad);
            jsonw_wave_lds_order();  // the run is assembled
            if (hi > lo && hi - lo <= kJsonwSpanLds) {
                const uintptr_t d0 = (uintptr_t)(e.out + lo), d1 = (uintptr_t)(e.out + hi), grid0 = d0 - shift;
                for (uint32_t b = 16 * lane; grid0 + b < d1; b += 16 * 64) {
                    const uintptr_t to = grid0 + b;
                    if (to >= d0 && to + 16 <= d1) {
                        *(OXH_JSONW_GLOBAL JsonwBlock16*)to = *(const JsonwBlock16*)&spans[wave][b];
                    } else {  // the block holds the run's head or tail: only the bytes inside
                        for (uint32_t k = 0; k < 16; ++k)
                            if (to + k >= d0 && to + k < d1) *(OXH_JSONW_GLOBAL uint8_t*)(to + k) = spans[wave][b + k];
                    }
                }
            } else {
                bad |= kJsonwErrPlace;  // the starts are not those of neighbours
            }
            jsonw_wave_lds_order();  // the run is stored: the next one may overwrite it
            todo &= ~run;
        }
        // 2. The rows of kJsonwLongCell bytes and more, straight to the output: their long cells are the whole wave's.
        const bool long_row = live && len >= kJsonwLongCell;
        if (__ballot(long_row)) jsonw_emit_row<false>(a, e, e.out + at, long_row, i, len, lane, spans[wave], bad);
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJsonwErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oxh

namespace {

namespace csvtext = oxh::csvtext;
namespace jsontext = oxh::jsontext;
using oxh::cols::is_bytes;

constexpr uint64_t kMaxWriteRows = 1ull << 40;

uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
unsigned row_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, oxh::kJsonwMaxGroups); }

struct WriteArgs {
    uint64_t nrows;
    uint32_t ncols;
    const uint32_t* types;
    const uint32_t* kinds;
    const void* const* values;
    const void* const* offsets;
    const uint8_t* const* validity;
    const uint64_t* bit_offsets;
    const uint8_t* names;
    const uint64_t* name_offsets;
    uint32_t flags;
    uint8_t* out;
    uint64_t capacity;
    uint64_t* out_bytes;
    uint64_t* stats4;
};

bool known_type(uint32_t t) { return t >= OXH_CSV_INT64 && t <= OXH_CSV_STRING64; }
uint32_t kind_of(uint32_t type) {
    return type == OXH_CSV_BOOL ? OXH_COL_BOOL : type == OXH_CSV_STRING ? OXH_COL_BYTES32 : type == OXH_CSV_STRING64 ? OXH_COL_BYTES64 : OXH_COL_FIXED8;
}

// "" when the arguments are well formed, else what is wrong with them, in the header's order.
std::string write_error(const WriteArgs& a, bool host) {
    if (!a.types || !a.kinds || !a.values || !a.offsets || !a.validity || !a.bit_offsets)
        return "types, kinds, values, offsets, validity or bit_offsets is NULL";
    if (a.ncols == 0) return "ncols is 0";
    if (a.flags & ~(uint32_t)OXH_JSON_ARRAY) return "unknown flags";
    for (uint32_t c = 0; c < a.ncols; ++c)
        if (!known_type(a.types[c])) return "column " + std::to_string(c) + " has unknown type " + std::to_string(a.types[c]);
    for (uint32_t c = 0; c < a.ncols; ++c)
        if (a.kinds[c] != kind_of(a.types[c]))
            return "column " + std::to_string(c) + " of type " + std::to_string(a.types[c]) + " has kind " + std::to_string(a.kinds[c]) +
                   ", not " + std::to_string(kind_of(a.types[c]));
    if (!a.name_offsets) return "name_offsets is NULL";
    for (uint32_t c = 0; c < a.ncols; ++c)
        if (a.name_offsets[c + 1] < a.name_offsets[c]) return "name_offsets decrease at column " + std::to_string(c);
    if (!a.names && a.name_offsets[a.ncols] > a.name_offsets[0]) return "names is NULL";
    if (!a.out_bytes || !a.stats4) return "out_bytes or stats4 is NULL";
    if (a.nrows > kMaxWriteRows) return "more than 2^40 rows";
    for (uint32_t c = 0; c < a.ncols && a.nrows; ++c) {
        const std::string what = oxh::cols::column_error("column " + std::to_string(c), a.kinds[c], a.values[c], a.offsets[c], a.nrows, host);
        if (!what.empty()) return what;
    }
    return "";
}

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// One call over device-resident columns, in two steps: measure() knows the file's bytes and the stats, emit() writes
// them. The lease (lengths, counts, starts, first slots, the scans' sums, the control words, the column table and
// the keys' text) lives as long as the call; the deferred cells' list and slots are a block of the call's own.
struct WriteCall {
    explicit WriteCall(hipStream_t stream) : st(stream), lease(stream) {}
    ~WriteCall() {
        (void)hipStreamSynchronize(st);
        if (d_defer) (void)hipFree(d_defer);
    }
    hipStream_t st;
    oxh::ScratchLease lease;
    uint8_t* d_defer = nullptr;
    oxh::JsonwArgs args{};
    oxh::JsonwEmit em{};
    unsigned long long *d_ctrl = nullptr, *h_ctrl = nullptr;
    uint8_t head[2] = {0, 0};  // the bytes in front of row 0: '[' of the array form, "[]" when it has no rows
    uint64_t head_bytes = 0, row_bytes = 0, ndeferred = 0;
    uint64_t stats[4] = {0, 0, 0, 0};

    int measure(const WriteArgs& a, const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                const uint64_t* bits);
    int emit(uint8_t* d_out);
};

int WriteCall::measure(const WriteArgs& a, const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                       const uint64_t* bits) {
    const uint64_t n = a.nrows;
    const bool array = (a.flags & OXH_JSON_ARRAY) != 0;
    if (array) head[0] = '[', head[1] = ']', head_bytes = n ? 1 : 2;
    if (n == 0) return OXH_OK;  // "[]", or nothing
    std::vector<uint8_t> keys;
    std::vector<uint64_t> key_at(a.ncols + 1, 0);
    uint64_t names_escaped = 0;
    for (uint32_t c = 0; c < a.ncols; ++c) {
        const uint64_t len = a.name_offsets[c + 1] - a.name_offsets[c];
        names_escaped += jsontext::key_text(len ? a.names + a.name_offsets[c] : nullptr, len, c == 0, keys);
        key_at[c + 1] = keys.size();
        if (key_at[c + 1] - key_at[c] >= oxh::kJsonwMaxRowText) return fail(OXH_ERR_INVALID, "json write: the text of one row is 2^32 bytes or more");
    }
    bool floats = false;
    for (uint32_t c = 0; c < a.ncols; ++c) floats |= a.types[c] == OXH_CSV_FLOAT64;
    // the small block, pinned and on the device: [ctrl | total of the lengths | total of the counts | columns | keys]
    const uint64_t cols_at = (oxh::kJsonwCtrlWords + 2) * 8, keys_at = cols_at + a.ncols * sizeof(oxh::JsonwCol);
    const uint64_t small = align256(keys_at + keys.size());
    // the lease: [small | lens u32 | counts u32 | starts u64 | first u64 | sums | sums]
    const uint64_t tiles = oxh::scan_tiles(n) + 1;
    const uint64_t lens_at = small, counts_at = lens_at + align256(n * 4), starts_at = counts_at + align256(n * 4);
    const uint64_t first_at = starts_at + align256(n * 8), sums_at = first_at + align256(n * 8), sums2_at = sums_at + align256(tiles * 8);
    const uint64_t total = sums2_at + align256(tiles * 8);
    void *lbase = nullptr, *pinned = nullptr;
    if (lease.get(total, &lbase) != hipSuccess || lease.pinned(small, &pinned) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "json write: " + std::to_string(total) + " B of row lengths and their scan");
    }
    uint8_t *b = (uint8_t*)lbase, *h = (uint8_t*)pinned;
    memset(h, 0, cols_at);
    oxh::JsonwCol* h_cols = (oxh::JsonwCol*)(h + cols_at);
    for (uint32_t c = 0; c < a.ncols; ++c) {
        h_cols[c].c.values = (const uint8_t*)d_values[c];
        h_cols[c].c.offsets = is_bytes(a.kinds[c]) ? (const uint8_t*)d_offsets[c] : nullptr;
        h_cols[c].c.validity = d_validity[c];
        h_cols[c].c.vbit = bits[2 * c], h_cols[c].c.nbit = bits[2 * c + 1];
        h_cols[c].c.kind = a.kinds[c], h_cols[c].c.order = 0;
        h_cols[c].key = b + keys_at + key_at[c];
        h_cols[c].type = a.types[c], h_cols[c].key_len = (uint32_t)(key_at[c + 1] - key_at[c]);
    }
    memcpy(h + keys_at, keys.data(), keys.size());
    h_ctrl = (unsigned long long*)h;
    d_ctrl = (unsigned long long*)b;
    uint32_t *d_lens = (uint32_t*)(b + lens_at), *d_counts = (uint32_t*)(b + counts_at);
    uint64_t *d_starts = (uint64_t*)(b + starts_at), *d_first = (uint64_t*)(b + first_at);
    unsigned long long *d_sums = (unsigned long long*)(b + sums_at), *d_sums2 = (unsigned long long*)(b + sums2_at);
    args = oxh::JsonwArgs{(const oxh::JsonwCol*)(b + cols_at), n, (uint64_t)keys.size(), a.ncols, array ? (uint32_t)',' : (uint32_t)'\n',
                          array ? (uint32_t)']' : (uint32_t)'\n'};
    auto column_error = [](unsigned long long e) -> int {
        if (e & oxh::kRowErrOffsets) return fail(OXH_ERR_INVALID, "json write: a byte column's offsets decrease or are negative");
        if (e & oxh::kRowErrValues) return fail(OXH_ERR_INVALID, "json write: a byte column has bytes but no values");
        if (e & oxh::kJsonwErrRowText) return fail(OXH_ERR_INVALID, "json write: the text of one row is 2^32 bytes or more");
        if (e) return fail(OXH_ERR_HIP, "json write: a deferred cell's place is outside its row's slots (did the columns change during the call?)");
        return OXH_OK;
    };
    HIP_TRY(hipMemcpyAsync(b, h, small, hipMemcpyHostToDevice, st));
    oxh::jsonw_length_kernel<<<row_grid(n), 256, 0, st>>>(args, d_lens, floats ? d_counts : nullptr, d_ctrl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, oxh::kJsonwCtrlWords * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int rc = column_error(h_ctrl[oxh::kJsonwErr]);
    if (rc) return rc;
    ndeferred = h_ctrl[oxh::kJsonwDeferred];
    if (ndeferred) {
        const uint64_t list_bytes = align256(ndeferred * 8), slot_bytes = ndeferred * oxh::kJsonwDeferSlot;
        if (hipMalloc(&d_defer, list_bytes + slot_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "json write: " + std::to_string(list_bytes + slot_bytes) + " B for " + std::to_string(ndeferred) + " deferred cells");
        }
        oxh::poison_device(d_defer, list_bytes + slot_bytes, st);
        uint64_t* d_list = (uint64_t*)d_defer;
        uint8_t* d_slots = d_defer + list_bytes;
        if ((rc = oxh::exclusive_scan_u32(d_counts, n, d_first, d_sums2, st))) return rc;
        oxh::jsonw_defer_list_kernel<<<row_grid(n), 256, 0, st>>>(args, d_counts, d_first, ndeferred, d_list, d_ctrl);
        HIP_TRY(hipGetLastError());
        std::vector<uint64_t> list(ndeferred);
        std::vector<uint8_t> slots(slot_bytes);
        HIP_TRY(hipMemcpyAsync(list.data(), d_list, ndeferred * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((rc = column_error(h_ctrl[oxh::kJsonwErr]))) return rc;
        for (uint64_t k = 0; k < ndeferred; ++k) csvtext::deferred_slot(list[k], slots.data() + k * oxh::kJsonwDeferSlot);
        HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), slot_bytes, hipMemcpyHostToDevice, st));
        oxh::jsonw_defer_add_kernel<<<row_grid(n), 256, 0, st>>>(d_counts, d_first, n, d_slots, ndeferred, d_lens, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));  // `slots` is pageable: the copy has read it
        em.defer_first = d_first, em.slots = d_slots, em.ndeferred = ndeferred;
    }
    if ((rc = oxh::exclusive_scan_u32(d_lens, n, d_starts, d_sums, st))) return rc;
    HIP_TRY(hipMemcpyAsync(h_ctrl + oxh::kJsonwCtrlWords, d_sums + oxh::scan_tiles(n), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = column_error(h_ctrl[oxh::kJsonwErr]))) return rc;
    row_bytes = h_ctrl[oxh::kJsonwCtrlWords];
    em.lens = d_lens, em.starts = d_starts, em.total = row_bytes;
    stats[1] = names_escaped + h_ctrl[oxh::kJsonwEscaped], stats[2] = ndeferred, stats[3] = h_ctrl[oxh::kJsonwNulls];
    STEP("json write: %llu rows x %u columns, %llu B, %llu deferred", (unsigned long long)n, a.ncols,
         (unsigned long long)(head_bytes + row_bytes), (unsigned long long)ndeferred);
    return OXH_OK;
}

// The head and the rows to d_out (head_bytes + row_bytes of device memory); complete on return.
int WriteCall::emit(uint8_t* d_out) {
    if (head_bytes) HIP_TRY(hipMemcpyAsync(d_out, head, head_bytes, hipMemcpyHostToDevice, st));
    if (args.nrows) {
        em.out = d_out + head_bytes;
        oxh::jsonw_emit_kernel<<<row_grid(args.nrows), 256, 0, st>>>(args, em, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (args.nrows && h_ctrl[oxh::kJsonwErr]) return fail(OXH_ERR_HIP, "json write: a row's text is not what was measured (did the columns change during the call?)");
    return OXH_OK;
}

void report(const WriteArgs& a, const WriteCall& call) {
    *a.out_bytes = call.head_bytes + call.row_bytes;
    a.stats4[0] = call.head_bytes + call.row_bytes;
    a.stats4[1] = call.stats[1], a.stats4[2] = call.stats[2], a.stats4[3] = call.stats[3];
}

int too_small(const WriteArgs& a, uint64_t need) {
    return fail(OXH_ERR_INVALID, "json write: out holds " + std::to_string(a.capacity) + " B, the file has " + std::to_string(need));
}

}  // namespace

extern "C" {

int oxh_write_json_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                          const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                          const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint32_t flags,
                          uint8_t* d_out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4, void* stream) {
    const WriteArgs a{nrows, ncols, types, kinds, d_values, d_offsets, d_validity, bit_offsets, names, name_offsets,
                      flags, d_out, capacity, out_bytes, stats4};
    const std::string what = write_error(a, false);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "json write: " + what);
    int rc = device_enter(ctx);
    if (rc) return rc;
    WriteCall call((hipStream_t)stream);
    if ((rc = call.measure(a, d_values, d_offsets, d_validity, bit_offsets))) return rc;
    const uint64_t need = call.head_bytes + call.row_bytes;
    if (d_out && capacity >= need && (rc = call.emit(d_out))) return rc;
    report(a, call);
    return d_out && capacity < need ? too_small(a, need) : OXH_OK;
}

int oxh_write_json_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                        const void* const* values, const void* const* offsets, const uint8_t* const* validity,
                        const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint32_t flags,
                        uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4) {
    const WriteArgs a{nrows, ncols, types, kinds, values, offsets, validity, bit_offsets, names, name_offsets,
                      flags, out, capacity, out_bytes, stats4};
    const std::string what = write_error(a, true);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "json write: " + what);
    int rc = device_enter(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    // One device block for the inputs: of every column only what its rows name (columns.hpp).
    oxh::cols::Staging plan;
    std::vector<oxh::cols::Staged> staged(ncols);
    for (uint32_t c = 0; c < ncols && nrows; ++c)
        staged[c] = plan.add_column(kinds[c], values[c], offsets[c], validity[c], bit_offsets[2 * c], bit_offsets[2 * c + 1], nrows);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    if (plan.total && hipMalloc(&d_in, plan.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "json write: " + std::to_string(plan.total) + " B for the columns on the device");
    }
    oxh::poison_device(d_in, plan.total, st);
    uint64_t need = 0;
    bool fits = false;
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : plan.pieces)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(d_in + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        std::vector<const void*> d_values(ncols, nullptr), d_offsets(ncols, nullptr);
        std::vector<const uint8_t*> d_validity(ncols, nullptr);
        std::vector<uint64_t> bits(2 * (size_t)ncols, 0);
        for (uint32_t c = 0; c < ncols && nrows; ++c) {
            d_values[c] = plan.values_at(d_in, staged[c]);
            d_offsets[c] = plan.offsets_at(d_in, staged[c]);
            d_validity[c] = plan.validity_at(d_in, staged[c]);
            bits[2 * c] = staged[c].vbit, bits[2 * c + 1] = staged[c].nbit;
        }
        WriteCall call(st);
        int r = call.measure(a, d_values.data(), d_offsets.data(), d_validity.data(), bits.data());
        if (r) return r;
        need = call.head_bytes + call.row_bytes;
        fits = out && capacity >= need;
        if (fits && need) {
            if (hipMalloc(&d_out, need) != hipSuccess) {
                (void)hipGetLastError();
                return fail(OXH_ERR_NOMEM, "json write: " + std::to_string(need) + " B for the file on the device");
            }
            oxh::poison_device(d_out, need, st);
            if ((r = call.emit(d_out))) return r;
            HIP_TRY(hipMemcpyAsync(out, d_out, need, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        report(a, call);
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (rc) return rc;
    return out && !fits ? too_small(a, need) : OXH_OK;
}

}  // extern "C"
