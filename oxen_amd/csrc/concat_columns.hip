// oxen_amd/csrc/concat_columns.hip -- row ranges of one or more frames written one after the other
// (oxh_concat_columns_*): `oxen df --vstack` (core/df/tabular.rs:449-463, polars' vertical concat) and
// `--slice` / `--head` / `--tail` / the page slice of every data-frame view (:571-636). Part p contributes its
// rows [first, first + count); the output columns are fresh Arrow buffers that start at bit / offset 0
// (DESIGN.md §4 "Concat"). A contiguous range needs no per-row gather: everything here is a copy.
//
// One call is, on one stream:
//   measure   (only with byte columns) concat_measure_kernel reads offsets[first] and offsets[first + count] of
//             every part and byte column; one read-back brings them: the host then knows every byte total and
//             where each part's bytes go. The sizes-only call and the call whose bytes do not fit stop here;
//   bits      concat_bits_kernel: one lane per 64-bit word of a bit-packed output (every column's validity, the
//             booleans' values). It finds the part of its first row by binary search in row_base and walks the
//             parts that overlap the word, up to 64 of them; a part's bits are read at any bit offset with a
//             funnel shift over nine bytes, a part without validity gives ones. The last word of an output is
//             stored byte by byte, only the bytes that hold rows;
//   fixed     concat_copy_kernel over the item list of the fixed-width values and the offsets: a copy item is one
//             window of kConcatPiece bytes on the DESTINATION's 16-byte grid, a lane per 16-byte block and
//             step -- a whole block is one unaligned 16-byte load and one aligned 16-byte store, a block cut
//             by the range's head or tail is written byte by byte, only the bytes inside the range; a rebase
//             item is kConcatOffsetPiece offsets, out = base + (offset - offsets[first]), which is also where
//             a negative or decreasing pair is found;
//   bytes     the same kernel over the item list of the byte columns' spans.
// The item lists are built on the host (concat_columns_host.hpp) and walked grid-stride under kConcatMaxGroups
// workgroups. There are no atomics and no read-modify-write on any output: every output word, offset and
// 16-byte block is produced by exactly one lane. Nothing outside a taken range is read.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "concat_columns_host.hpp"

using namespace oxh::capi;

namespace oxh {

constexpr unsigned kConcatMaxGroups = 2048;

struct ConcatProbe {  // one offset to read (measure): at NULL = none
    const uint8_t* at;
    uint64_t wide;  // 4 or 8
};

struct ConcatBits {
    const uint64_t* row_base;    // nparts + 1
    const concat::BitSrc* src;   // nstreams * nparts
    uint8_t* const* dst;         // nstreams
    uint64_t n, words;           // output rows; 64-bit words of one output
    uint32_t nparts, nstreams;
};

__global__ __launch_bounds__(256) void concat_measure_kernel(const ConcatProbe* probe, uint64_t n, int64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ConcatProbe p = probe[i];
    out[i] = !p.at ? 0 : p.wide == 4 ? (int64_t)(int32_t)ld32u(p.at) : (int64_t)ld64u(p.at);
}

// k (1..64) bits of a part from its row `at` on, in the low bits. The part holds `rows` rows: nothing past the
// byte of its last row is read.
__device__ __forceinline__ uint64_t concat_part_bits(const concat::BitSrc& s, uint64_t at, uint32_t k, uint64_t rows) {
    const uint64_t ones = k == 64 ? ~0ull : (1ull << k) - 1;
    if (!s.p) return ones;
    const uint64_t bit = s.bit + at, byte0 = bit >> 3, end = (s.bit + rows + 7) >> 3;
    const uint32_t sh = (uint32_t)(bit & 7);
    uint64_t lo = 0;
    if (byte0 + 8 <= end) {
        lo = ld64u(s.p + byte0);
    } else {
        for (uint64_t b = byte0; b < end; ++b) lo |= (uint64_t)s.p[b] << (8 * (b - byte0));
    }
    uint64_t v = lo >> sh;
    if (sh + k > 64) v |= (uint64_t)s.p[byte0 + 8] << (64 - sh);  // the ninth byte holds the part's row at + k - 1
    return v & ones;
}

__global__ __launch_bounds__(256) void concat_bits_kernel(ConcatBits a) {
    const uint64_t total = a.words * a.nstreams;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t s = i / a.words, w = i - s * a.words;
        const uint64_t row0 = w * 64, end = row0 + 64 < a.n ? row0 + 64 : a.n;
        uint32_t lo = 0, hi = a.nparts;  // row_base[lo] <= row0 < row_base[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.row_base[mid] <= row0) lo = mid;
            else hi = mid;
        }
        uint64_t word = 0, r = row0;
        for (uint32_t p = lo; r < end && p < a.nparts; ++p) {
            const uint64_t p0 = a.row_base[p], p1 = a.row_base[p + 1];
            if (p1 <= r) continue;  // an empty part
            const uint32_t k = (uint32_t)((p1 < end ? p1 : end) - r);
            word |= concat_part_bits(a.src[s * a.nparts + p], r - p0, k, p1 - p0) << (r - row0);
            r += k;
        }
        uint8_t* at = a.dst[s] + 8 * w;
        if (end - row0 == 64) {
            *reinterpret_cast<unsigned long long*>(at) = word;
        } else {
            for (uint64_t b = 0; b < ((end - row0 + 7) >> 3); ++b) at[b] = (uint8_t)(word >> (8 * b));
        }
    }
}

typedef uint32_t ConcatBlock16 __attribute__((ext_vector_type(4)));  // one 16-byte block
typedef ConcatBlock16 ConcatBlock16u __attribute__((aligned(1)));    // the same at any address
// The descriptors' pointers are global memory; saying so keeps the copies off the flat path.
#define OXH_GLOBAL __attribute__((address_space(1)))

// One workgroup per item and round.
__global__ __launch_bounds__(256) void concat_copy_kernel(const concat::Span* spans, const concat::Item* items, uint64_t nitems,
                                                          unsigned long long* ctrl) {
    unsigned long long bad = 0;
    for (uint64_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        const concat::Item item = items[it];
        const concat::Span s = spans[item.span];
        if (s.mode == 0) {
            const uintptr_t d0 = (uintptr_t)s.dst, d1 = d0 + s.n;
            const uintptr_t window = (d0 & ~(uintptr_t)15) + (uintptr_t)item.piece * concat::kConcatPiece;
            for (uint32_t b = threadIdx.x * 16; b < concat::kConcatPiece; b += 256 * 16) {
                const uintptr_t at = window + b;
                if (at >= d1) break;
                if (at >= d0 && at + 16 <= d1) {
                    const ConcatBlock16 v = *(const OXH_GLOBAL ConcatBlock16u*)(uintptr_t)(s.src + (at - d0));
                    *(OXH_GLOBAL ConcatBlock16*)at = v;
                } else {  // the block holds the range's head or tail: only the bytes inside
                    const uintptr_t from = at < d0 ? d0 : at, to = at + 16 < d1 ? at + 16 : d1;
                    for (uintptr_t x = from; x < to; ++x) *reinterpret_cast<uint8_t*>(x) = s.src[x - d0];
                }
            }
        } else {
            const uint64_t begin = (uint64_t)item.piece * concat::kConcatOffsetPiece;
            const uint64_t stop = begin + concat::kConcatOffsetPiece < s.n ? begin + concat::kConcatOffsetPiece : s.n;
            for (uint64_t j = begin + threadIdx.x; j < stop; j += 256) {
                int64_t cur, before;
                if (s.mode == 4) {
                    cur = (int32_t)ld32u(s.src + 4 * j);
                    before = j ? (int64_t)(int32_t)ld32u(s.src + 4 * (j - 1)) : cur;
                } else {
                    cur = (int64_t)ld64u(s.src + 8 * j);
                    before = j ? (int64_t)ld64u(s.src + 8 * (j - 1)) : cur;
                }
                int64_t v = cur;
                if (before < 0 || cur < before) {  // a bad pair: the cell before this offset has length 0
                    v = before;
                    bad |= kRowErrOffsets;
                }
                v = v < s.lo ? s.lo : v > s.hi ? s.hi : v;  // never outside the bytes the part brought
                const uint64_t out = s.base + (uint64_t)(v - s.lo);
                if (s.mode == 4) {
                    const int32_t o = (int32_t)out;
                    __builtin_memcpy(s.dst + 4 * j, &o, 4);
                } else {
                    __builtin_memcpy(s.dst + 8 * j, &out, 8);
                }
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(ctrl, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oxh

namespace {

using oxh::cols::is_bytes;
namespace concat = oxh::concat;

uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// The lease's device block and its pinned mirror, `bytes` each.
int lease_block(oxh::ScratchLease& lease, uint64_t bytes, uint8_t** d, uint8_t** h) {
    void *dv = nullptr, *hv = nullptr;
    if (lease.get(bytes, &dv) != hipSuccess || lease.pinned(bytes, &hv) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "concat: " + std::to_string(bytes) + " B of tables");
    }
    *d = (uint8_t*)dv, *h = (uint8_t*)hv;
    return OXH_OK;
}

// plan.byte_span from the device: [probes | answers] in the lease, one launch, one read-back.
int concat_measure(const concat::Args& a, concat::Plan& plan, oxh::ScratchLease& lease, hipStream_t st) {
    const uint64_t n = 2 * plan.byte_span.size();
    if (!n) return OXH_OK;
    const uint64_t out_at = align16(n * sizeof(oxh::ConcatProbe));
    uint8_t *d = nullptr, *h = nullptr;
    int rc = lease_block(lease, out_at + n * 8, &d, &h);
    if (rc) return rc;
    oxh::ConcatProbe* probe = (oxh::ConcatProbe*)h;
    for (size_t j = 0; j < plan.byte_cols.size(); ++j)
        for (uint32_t p = 0; p < a.nparts; ++p) {
            const uint32_t c = plan.byte_cols[j], ow = oxh::cols::offset_width(a.kinds[c]);
            const uint64_t cnt = concat::count_of(a, p);
            const uint8_t* off = cnt ? (const uint8_t*)a.offsets[(size_t)p * a.ncols + c] + concat::first_of(a, p) * ow : nullptr;
            probe[2 * (j * a.nparts + p)] = {off, ow};
            probe[2 * (j * a.nparts + p) + 1] = {off ? off + cnt * ow : nullptr, ow};
        }
    HIP_TRY(hipMemcpyAsync(d, h, n * sizeof(oxh::ConcatProbe), hipMemcpyHostToDevice, st));
    oxh::concat_measure_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const oxh::ConcatProbe*)d, n, (int64_t*)(d + out_at));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h + out_at, d + out_at, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t* got = (const int64_t*)(h + out_at);
    for (size_t k = 0; k < plan.byte_span.size(); ++k) plan.byte_span[k] = {got[2 * k], got[2 * k + 1]};
    return OXH_OK;
}

// Every output, to device buffers; complete on return. plan.byte_span and the sizes are known and fit; n > 0.
// bad_pairs: a pair of offsets inside a taken range was negative or decreased.
int concat_write(const concat::Args& a, concat::Plan& plan, oxh::ScratchLease& lease, hipStream_t st, void* const* d_out_values,
                 void* const* d_out_offsets, uint8_t* const* d_out_validity, bool& bad_pairs) {
    plan.make_bits(a);
    plan.make_items(a, d_out_values, d_out_offsets);
    const uint32_t nstreams = plan.nstreams(a);
    const uint64_t nfixed = plan.fixed_items.size(), nbytes = plan.byte_items.size();
    const uint64_t bits_at = align16((a.nparts + 1ull) * 8), dst_at = bits_at + align16(plan.bits.size() * sizeof(concat::BitSrc));
    const uint64_t spans_at = dst_at + align16(nstreams * 8ull), items_at = spans_at + align16(plan.spans.size() * sizeof(concat::Span));
    const uint64_t ctrl_at = items_at + (nfixed + nbytes) * sizeof(concat::Item), bytes = ctrl_at + 16;
    uint8_t *d = nullptr, *h = nullptr;
    int rc = lease_block(lease, bytes, &d, &h);
    if (rc) return rc;
    memcpy(h, plan.row_base.data(), (a.nparts + 1ull) * 8);
    memcpy(h + bits_at, plan.bits.data(), plan.bits.size() * sizeof(concat::BitSrc));
    uint8_t** dst = (uint8_t**)(h + dst_at);
    for (uint32_t c = 0; c < a.ncols; ++c) dst[c] = d_out_validity[c];
    for (size_t j = 0; j < plan.bool_cols.size(); ++j) dst[a.ncols + j] = (uint8_t*)d_out_values[plan.bool_cols[j]];
    if (!plan.spans.empty()) memcpy(h + spans_at, plan.spans.data(), plan.spans.size() * sizeof(concat::Span));
    if (nfixed) memcpy(h + items_at, plan.fixed_items.data(), nfixed * sizeof(concat::Item));
    if (nbytes) memcpy(h + items_at + nfixed * sizeof(concat::Item), plan.byte_items.data(), nbytes * sizeof(concat::Item));
    memset(h + ctrl_at, 0, 16);
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    oxh::ConcatBits b{(const uint64_t*)d, (const concat::BitSrc*)(d + bits_at), (uint8_t* const*)(d + dst_at), plan.n, (plan.n + 63) / 64,
                      a.nparts, nstreams};
    auto groups = [](uint64_t n) { return (unsigned)(n < oxh::kConcatMaxGroups ? n : oxh::kConcatMaxGroups); };
    oxh::concat_bits_kernel<<<groups((b.words * nstreams + 255) / 256), 256, 0, st>>>(b);
    HIP_TRY(hipGetLastError());
    const concat::Span* spans = (const concat::Span*)(d + spans_at);
    const concat::Item* items = (const concat::Item*)(d + items_at);
    unsigned long long* ctrl = (unsigned long long*)(d + ctrl_at);
    if (nfixed) {
        oxh::concat_copy_kernel<<<groups(nfixed), 256, 0, st>>>(spans, items, nfixed, ctrl);
        HIP_TRY(hipGetLastError());
    }
    if (nbytes) {
        oxh::concat_copy_kernel<<<groups(nbytes), 256, 0, st>>>(spans, items + nfixed, nbytes, ctrl);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h + ctrl_at, ctrl, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bad_pairs = *(const unsigned long long*)(h + ctrl_at) != 0;
    STEP("concat: %llu rows of %u parts, %u bit streams, %llu + %llu items", (unsigned long long)plan.n, a.nparts, nstreams,
         (unsigned long long)nfixed, (unsigned long long)nbytes);
    return OXH_OK;
}

// What both forms do before they need a device. `done`: no output rows, nothing left to do.
int concat_enter(oxh_ctx* ctx, const concat::Args& a, bool host, bool& done) {
    done = false;
    const std::string what = concat::argument_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "concat: " + what);
    uint64_t n = 0;
    for (uint32_t p = 0; p < a.nparts; ++p) n += concat::count_of(a, p);
    if (n == 0) {
        bool offsets = false;  // a byte column's single 0 is device memory in the device form
        for (uint32_t c = 0; c < a.ncols && !concat::sizes_only(a); ++c) {
            if (!is_bytes(a.kinds[c])) continue;
            if (host) memset(a.out_offsets[c], 0, oxh::cols::offset_width(a.kinds[c]));
            offsets = true;
        }
        if (host || !offsets) {
            memset(a.value_bytes, 0, a.ncols * sizeof(uint64_t));
            *a.written = concat::sizes_only(a) ? 0 : 1;
            done = true;
            return OXH_OK;
        }
    }
    return device_enter(ctx);
}

}  // namespace

extern "C" {

int oxh_concat_columns_device(oxh_ctx* ctx, uint32_t nparts, uint32_t ncols, const uint32_t* kinds, const void* const* d_values,
                              const void* const* d_offsets, const uint8_t* const* d_validity, const uint64_t* bit_offsets,
                              const uint64_t* part_rows, const uint64_t* first, const uint64_t* count, const uint64_t* value_capacity,
                              void* const* d_out_values, void* const* d_out_offsets, uint8_t* const* d_out_validity,
                              uint64_t* value_bytes, uint32_t* written, void* stream) {
    const concat::Args a{nparts, ncols, kinds, d_values, d_offsets, d_validity, bit_offsets, part_rows, first, count, value_capacity,
                         d_out_values, d_out_offsets, d_out_validity, value_bytes, written};
    bool done = false;
    int rc = concat_enter(ctx, a, false, done);
    if (rc || done) return rc;
    hipStream_t st = (hipStream_t)stream;
    concat::Plan plan(a);
    if (plan.n == 0) {  // outputs given: the byte columns' single offset
        for (uint32_t c : plan.byte_cols) HIP_TRY(hipMemsetAsync(d_out_offsets[c], 0, oxh::cols::offset_width(kinds[c]), st));
        HIP_TRY(hipStreamSynchronize(st));
        memset(value_bytes, 0, ncols * sizeof(uint64_t));
        *written = 1;
        return OXH_OK;
    }
    oxh::ScratchLease lease(st);
    if ((rc = concat_measure(a, plan, lease, st))) return rc;
    const std::string what = plan.make_sizes(a);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "concat: " + what);
    const bool fits = !concat::sizes_only(a) && plan.fits(a);
    bool bad_pairs = false;
    if (fits && (rc = concat_write(a, plan, lease, st, d_out_values, d_out_offsets, d_out_validity, bad_pairs))) return rc;
    memcpy(value_bytes, plan.need.data(), ncols * sizeof(uint64_t));
    *written = fits ? 1 : 0;
    if (plan.bad_span || bad_pairs) return fail(OXH_ERR_INVALID, "concat: a byte column's offsets decrease or are negative inside a taken range");
    return OXH_OK;
}

int oxh_concat_columns_host(oxh_ctx* ctx, uint32_t nparts, uint32_t ncols, const uint32_t* kinds, const void* const* values,
                            const void* const* offsets, const uint8_t* const* validity, const uint64_t* bit_offsets,
                            const uint64_t* part_rows, const uint64_t* first, const uint64_t* count, const uint64_t* value_capacity,
                            void* const* out_values, void* const* out_offsets, uint8_t* const* out_validity, uint64_t* value_bytes,
                            uint32_t* written) {
    const concat::Args a{nparts, ncols, kinds, values, offsets, validity, bit_offsets, part_rows, first, count, value_capacity,
                         out_values, out_offsets, out_validity, value_bytes, written};
    bool done = false;
    int rc = concat_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    concat::Plan sizes(a);  // the host reads its own offsets: the sizes need no device work
    concat::host_spans(a, sizes);
    const std::string what = sizes.make_sizes(a);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "concat: " + what);
    const bool fits = !concat::sizes_only(a) && sizes.fits(a);
    if (!fits) {
        memcpy(value_bytes, sizes.need.data(), ncols * sizeof(uint64_t));
        *written = 0;
        return OXH_OK;
    }
    // One device block for the inputs: of every part and column only the taken range (columns.hpp). The
    // staged parts start at row 0, so the device path sees whole parts of `count` rows.
    const concat::HostStaging in(a);
    const concat::OutBlock where(a, sizes.n, sizes.need.data());
    uint8_t *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_in, in.block.total + 16) != hipSuccess || hipMalloc(&d_out, where.total + 16) != hipSuccess) {
        (void)hipGetLastError();
        if (d_in) (void)hipFree(d_in);
        return fail(OXH_ERR_NOMEM, "concat: " + std::to_string(in.block.total + where.total) + " B for the columns on the device");
    }
    oxh::poison_device(d_in, in.block.total + 16, st), oxh::poison_device(d_out, where.total + 16, st);
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : in.block.pieces)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(d_in + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        const size_t cells = (size_t)nparts * ncols;
        std::vector<const void*> d_values(cells), d_offsets(cells);
        std::vector<const uint8_t*> d_validity(cells);
        std::vector<uint64_t> bits(2 * cells, 0), rows(nparts);
        for (size_t k = 0; k < cells; ++k) {
            d_values[k] = in.block.values_at(d_in, in.staged[k]);
            d_offsets[k] = in.block.offsets_at(d_in, in.staged[k]);
            d_validity[k] = in.block.validity_at(d_in, in.staged[k]);
            bits[2 * k] = in.staged[k].vbit, bits[2 * k + 1] = in.staged[k].nbit;
        }
        for (uint32_t p = 0; p < nparts; ++p) rows[p] = concat::count_of(a, p);
        const concat::Args dev{nparts, ncols, kinds, d_values.data(), d_offsets.data(), d_validity.data(), bits.data(), rows.data(),
                               nullptr, nullptr, value_capacity, nullptr, nullptr, nullptr, value_bytes, written};
        concat::Plan plan(dev);
        plan.byte_span = sizes.byte_span;  // a staged byte column keeps its offsets: its values pointer is rebased
        (void)plan.make_sizes(dev);
        std::vector<void*> o_values(ncols), o_offsets(ncols);
        std::vector<uint8_t*> o_validity(ncols);
        for (uint32_t c = 0; c < ncols; ++c) {
            o_validity[c] = d_out + where.at[3 * c];
            o_values[c] = d_out + where.at[3 * c + 1];
            o_offsets[c] = d_out + where.at[3 * c + 2];
        }
        oxh::ScratchLease lease(st);
        bool bad_pairs = false;
        int r = concat_write(dev, plan, lease, st, o_values.data(), o_offsets.data(), o_validity.data(), bad_pairs);
        if (r) return r;
        if (bad_pairs) return fail(OXH_ERR_HIP, "concat: the offsets changed during the call");
        for (uint32_t c = 0; c < ncols; ++c) {
            HIP_TRY(hipMemcpyAsync(out_validity[c], o_validity[c], concat::bitmap_bytes(sizes.n), hipMemcpyDeviceToHost, st));
            if (sizes.need[c]) HIP_TRY(hipMemcpyAsync(out_values[c], o_values[c], sizes.need[c], hipMemcpyDeviceToHost, st));
            if (is_bytes(kinds[c]))
                HIP_TRY(hipMemcpyAsync(out_offsets[c], o_offsets[c], (sizes.n + 1) * oxh::cols::offset_width(kinds[c]), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (rc) return rc;
    memcpy(value_bytes, sizes.need.data(), ncols * sizeof(uint64_t));
    *written = 1;
    return OXH_OK;
}

}  // extern "C"
