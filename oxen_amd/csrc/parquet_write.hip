// oxen_amd/csrc/parquet_write.hip -- typed Arrow columns in HBM to the bytes of a Parquet file (oxh_write_parquet_*):
// `write_df`'s parquet arm (core/df/tabular.rs:1508-1517). The format -- uncompressed DataPage V1 pages, PLAIN values,
// RLE / bit-packed definition levels, statistics per column chunk -- is stated in include/oxen_hash.h "Parquet"
// (DESIGN.md §4 "Parquet"). Rows are cut into tiles of 1 024; a wave owns one (tile, column) at a time:
//   measure  pqw_measure_kernel: per (tile, column) the rows that are not null (popcounts of the wave's validity
//            ballots), the value bytes (8 a cell, 4 + length a string cell, the count for booleans) and the min / max
//            of the numeric columns (NaNs left out) by wave reductions -- no atomics, the same bits every run. The
//            tile table comes down in one copy;
//   plan     parquet_host.hpp, on the host: pages, row groups, every PageHeader's Thrift bytes with the levels'
//            length and run header behind it, every page's place in the file, per (tile, column) its page, the valid
//            rows and value bytes of the page in front of it, and the footer. The plan goes up in one copy; the magic
//            and the footer go from host memory to their places in the file, two small copies of their own;
//   emit     pqw_emit_kernel: the page's first tile copies the page's head. Every tile writes its 128 bytes of
//            validity (pages with a null) and compacts its values: the rank of a row among the valid rows of its page
//            is the tile's base from the plan, plus the popcounts of the steps in front of it, plus mbcnt inside the
//            step's ballot. Fixed-width cells go to their ranks in the wave's LDS, at the destination's own
//            misalignment, and are stored 16 bytes a lane on the destination's 16-byte grid (a page starts at any
//            byte: header sizes vary); a column without validity skips LDS, its tile is one straight shifted copy,
//            16 unaligned source bytes a lane to an aligned block. Boolean values leave as single bytes, a lane
//            each (at most 129 a tile), not as blocks: their bits are compacted step by step (a byte per valid row
//            in LDS, one ballot), appended to a bit accumulator that starts with the bits of the page's earlier rows
//            that share the tile's first byte (at most 7, carried by the plan), so every byte has one writer. String
//            cells: a wave scan of 4 + length places them; the cells below kPqLongCell bytes are assembled in LDS in runs of
//            neighbouring rows whose span fits kPqSpanLds and stored as aligned blocks; a longer cell is copied by
//            the whole wave, 8 bytes a lane.
// Every byte of the file is written by exactly one place (the head, a tile's levels, a tile's values, the host's
// magic and footer), so the result does not depend on what the output or the scratch held. Every store is checked
// against the page's own sizes first: columns that change during the call set the error word, they do not write
// outside. No workgroup waits for another; launches order the steps.
#include "parquet_device.hpp"

using namespace oxh::capi;
namespace pq = oxh::parquet;

namespace oxh {

constexpr uint32_t kPqLongCell = 512;      // a string cell of this many bytes (its length word included) and more is the whole wave's
static_assert(pq::kTileRows * 8 <= kPqSpanLds, "a tile of 8-byte cells fits the wave's LDS");

__device__ __forceinline__ unsigned long long pqw_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
    return v;
}

// ---------------------------------------------------------------- measure
__global__ __launch_bounds__(256) void pqw_measure_kernel(const PqArgs a, pq::Tile* __restrict__ tiles, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t items = a.ntiles * a.ncols, nwaves = (uint64_t)gridDim.x * 4;
    unsigned long long bad = 0;
    for (uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += nwaves) {  // uniform in the wave
        const PqCol& pc = a.cols[item % a.ncols];
        if (pq::is_list(pc.type)) continue;  // parquet_write_lists.hip fills a list column's tiles
        const uint64_t r0 = (item / a.ncols) * pq::kTileRows;
        uint32_t valid = 0;
        unsigned long long bytes = 0;
        long long imin = INT64_MAX, imax = INT64_MIN;
        double dmin = __builtin_huge_val(), dmax = -__builtin_huge_val();
        bool any = false;
        uint32_t tail = 0;
        for (uint32_t s = 0; s < 16 && r0 + 64 * s < a.nrows; ++s) {
            const uint64_t r = r0 + 64 * s + lane;
            const bool live = r < a.nrows && pqw_present(pc.c, r);
            const unsigned long long mask = __ballot(live);
            valid += (uint32_t)__popcll(mask);
            if (pc.type == OXH_CSV_BOOL) {  // uniform: the values of the tile's last 7 valid rows, the last one in bit 0
                const unsigned long long vals = __ballot(live && row_bit(pc.c.values, pc.c.vbit + r));
                tail = pq::bool_tail(tail, mask, vals);
                continue;
            }
            if (!live) continue;
            if (pc.type == OXH_CSV_INT64) {
                const long long v = (long long)ld64u(pc.c.values + 8 * r);
                imin = v < imin ? v : imin, imax = v > imax ? v : imax;
            } else if (pc.type == OXH_CSV_FLOAT64) {
                const double v = __longlong_as_double((long long)ld64u(pc.c.values + 8 * r));
                if (v == v) any = true, dmin = v < dmin ? v : dmin, dmax = v > dmax ? v : dmax;
            } else if (pc.type != OXH_CSV_BOOL) {
                uint64_t start = 0;
                const uint64_t cell = row_cell(pc.c, r, start, bad);
                if (cell >= pq::kMaxCell)
                    bad |= kPqErrCell;
                else
                    bytes += 4 + cell;
            }
        }
        pq::Tile t{};
        t.valid = valid;
        if (pc.type == OXH_CSV_INT64) {
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                const long long lo = __shfl_xor(imin, off, 64), hi = __shfl_xor(imax, off, 64);
                imin = lo < imin ? lo : imin, imax = hi > imax ? hi : imax;
            }
            t.value_bytes = 8ull * valid, t.min = (uint64_t)imin, t.max = (uint64_t)imax, t.has_minmax = valid != 0;
        } else if (pc.type == OXH_CSV_FLOAT64) {
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                const double lo = __longlong_as_double(__shfl_xor(__double_as_longlong(dmin), off, 64));
                const double hi = __longlong_as_double(__shfl_xor(__double_as_longlong(dmax), off, 64));
                dmin = lo < dmin ? lo : dmin, dmax = hi > dmax ? hi : dmax;
            }
            // which zero of +-0.0 a reduction keeps does not matter: the host writes a zero min as -0.0, a zero max as +0.0
            t.value_bytes = 8ull * valid, t.min = (uint64_t)__double_as_longlong(dmin), t.max = (uint64_t)__double_as_longlong(dmax);
            t.has_minmax = __ballot(any) != 0;
        } else if (pc.type == OXH_CSV_BOOL) {
            t.value_bytes = valid, t.min = tail;
        } else {
            t.value_bytes = pqw_wave_sum(bytes);
        }
        if (lane == 0) tiles[item] = t;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- emit
// One 64-row step of a tile: the rows that are not null, as the lane's flag and the wave's ballot; the step's 8
// bytes of the page's bit-packed levels go to their place (`room`: the level bytes the tile owns; rows behind the
// frame's last are 0 bits, the pad).
__device__ __forceinline__ unsigned long long pqw_step(const PqArgs& a, const RowCol& c, uint64_t r, uint32_t s, uint8_t* levels, uint32_t room,
                                                       unsigned lane, bool& live) {
    live = r < a.nrows && pqw_present(c, r);
    const unsigned long long mask = __ballot(live);
    if (lane < 8 && 8 * s + lane < room) levels[8 * s + lane] = (uint8_t)(mask >> (8 * lane));
    return mask;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void pqw_emit_kernel(const PqArgs a, const PqEmit e, unsigned long long* __restrict__ ctrl) {
    __shared__ __attribute__((aligned(16))) uint8_t spans[4][kPqSpanLds + 16];
    const unsigned lane = threadIdx.x & 63;
    uint8_t* const stage = spans[threadIdx.x >> 6];
    const uint64_t items = a.ntiles * a.ncols, nwaves = (uint64_t)gridDim.x * 4;
    unsigned long long bad = 0;
    for (uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += nwaves) {  // uniform in the wave
        const PqCol& pc = a.cols[item % a.ncols];
        if (pq::is_list(pc.type)) continue;  // parquet_write_lists.hip writes a list column's pages
        const uint64_t tile = item / a.ncols, r0 = tile * pq::kTileRows;
        const pq::Place pl = e.places[item];
        if (pl.page >= e.npages) {
            bad |= kPqErrPlace;
            continue;
        }
        const pq::Page pg = e.pages[pl.page];
        if (tile < pg.tile0 || r0 < pg.row0 || r0 >= pg.row0 + pg.rows || pl.rank_base > pg.nvalid) {
            bad |= kPqErrPlace;
            continue;
        }
        uint8_t* const page_out = e.out + pg.file_at;
        if (tile == pg.tile0) copy_span_wave(page_out, e.blob + pg.head_src, pg.head_len, lane);
        const uint64_t level_at = (tile - pg.tile0) * (pq::kTileRows / 8);
        uint8_t* const levels = page_out + pg.head_len + level_at;
        const uint64_t level_left = level_at < pg.level_bytes ? pg.level_bytes - level_at : 0;
        const uint32_t room = level_left < pq::kTileRows / 8 ? (uint32_t)level_left : (uint32_t)(pq::kTileRows / 8);
        uint8_t* const vals = page_out + pg.head_len + pg.level_bytes;
        const uint32_t steps = a.nrows - r0 < pq::kTileRows ? (uint32_t)((a.nrows - r0 + 63) / 64) : 16u;
        bool live;
        if (pg.dict_width) {
            // a page of a dictionary chunk (OXH_PARQUET_DICTIONARY): the levels here, and by the page's first tile the
            // width byte and the run header of its index stream -- by the chunk's first tile the dictionary page's
            // header too; the entries and the packed indices are parquet_dict.hip's
            if (tile == pg.tile0) {
                if (pl.page > 0 && pg.dict_page == pl.page - 1) {
                    const pq::Page dp = e.pages[pg.dict_page];
                    copy_span_wave(e.out + dp.file_at, e.blob + dp.head_src, dp.head_len, lane);
                }
                const uint64_t run = ((((uint64_t)pg.nvalid + 7) / 8) << 1) | 1;
                const uint32_t nrun = pg.nvalid ? pq::varint_len(run) : 0;
                if (1 + nrun > pg.values_bytes)
                    bad |= kPqErrPlace;
                else if (lane == 0)
                    vals[0] = (uint8_t)pg.dict_width;
                else if (lane <= nrun)
                    vals[lane] = (uint8_t)(((run >> (7 * (lane - 1))) & 0x7F) | (lane < nrun ? 0x80 : 0));
            }
            for (uint32_t s = 0; s < steps && room; ++s) pqw_step(a, pc.c, r0 + 64 * s + lane, s, levels, room, lane, live);
        } else if ((pc.type == OXH_CSV_INT64 || pc.type == OXH_CSV_FLOAT64) && !pc.c.validity) {
            // a column without validity: every row is its own rank, the tile is one straight shifted copy
            const uint64_t rows = a.nrows - r0 < pq::kTileRows ? a.nrows - r0 : pq::kTileRows;
            if (8ull * (pl.rank_base + rows) <= pg.values_bytes)
                pqw_copy_span(vals + 8ull * pl.rank_base, pc.c.values + 8 * r0, 8 * rows, lane);
            else
                bad |= kPqErrPlace;
        } else if (pc.type == OXH_CSV_INT64 || pc.type == OXH_CSV_FLOAT64) {
            // the tile's valid cells to their ranks in LDS, then the span in aligned blocks
            uint8_t* const d = vals + 8ull * pl.rank_base;
            const uint32_t shift = (uint32_t)((uintptr_t)d & 15);
            uint32_t cnt = 0;
            for (uint32_t s = 0; s < steps; ++s) {
                const uint64_t r = r0 + 64 * s + lane;
                const unsigned long long mask = pqw_step(a, pc.c, r, s, levels, room, lane, live);
                if (live) {
                    const uint64_t v = ld64u(pc.c.values + 8 * r);
                    __builtin_memcpy(stage + shift + 8 * (cnt + pqw_below(mask)), &v, 8);
                }
                cnt += (uint32_t)__popcll(mask);
            }
            pqw_wave_lds_order();  // the tile is assembled
            if (8ull * (pl.rank_base + cnt) <= pg.values_bytes)
                pqw_store_span(d, 8ull * cnt, stage, lane);
            else
                bad |= kPqErrPlace;
            pqw_wave_lds_order();  // the span is stored: the next item may overwrite it
        } else if (pc.type == OXH_CSV_BOOL) {
            uint8_t* const tmp = stage;                       // a byte per valid row of a step
            uint64_t* const words = (uint64_t*)(stage + 64);  // the tile's bits: at most 7 + 1 024
            // the bits of the page's earlier valid rows that share the tile's first byte: the plan carries them from
            // the tiles in front (the measure kernel leaves every tile's last 7), so no tile reads another's rows
            const uint32_t need = pl.rank_base & 7;
            unsigned long long acc = pl.byte_base & ((1ull << need) - 1);
            uint32_t accbits = need, nwords = 0;
            uint32_t cnt_all = 0;
            for (uint32_t s = 0; s < steps; ++s) {
                const uint64_t r = r0 + 64 * s + lane;
                const unsigned long long mask = pqw_step(a, pc.c, r, s, levels, room, lane, live);
                const bool bit = live && row_bit(pc.c.values, pc.c.vbit + r);
                const uint32_t cnt = (uint32_t)__popcll(mask);
                unsigned long long comp;
                if (mask == ~0ull) {
                    comp = __ballot(bit);
                } else {
                    if (live) tmp[pqw_below(mask)] = bit ? 1 : 0;
                    pqw_wave_lds_order();
                    comp = __ballot(lane < cnt && tmp[lane & 63] != 0);
                    pqw_wave_lds_order();
                }
                acc |= comp << accbits;  // accbits < 64
                if (accbits + cnt >= 64) {
                    if (lane == 0) words[nwords] = acc;
                    ++nwords;
                    acc = accbits ? comp >> (64 - accbits) : 0ull;
                    accbits = accbits + cnt - 64;
                } else {
                    accbits += cnt;
                }
                cnt_all += cnt;
            }
            if (accbits) {
                if (lane == 0) words[nwords] = acc;
                ++nwords;
            }
            pqw_wave_lds_order();  // the tile's bits are in LDS
            // byte k of the page's values is written by the tile that holds its last bit (the page's last bit for the
            // last byte): the tile's bytes run from the one rank_base falls into
            const uint64_t b1 = (uint64_t)pl.rank_base + cnt_all;
            if (cnt_all) {
                const uint64_t k0 = pl.rank_base >> 3, k1 = b1 >= pg.nvalid ? ((uint64_t)pg.nvalid + 7) >> 3 : b1 >> 3;
                if (b1 > pg.nvalid || k1 > pg.values_bytes) {
                    bad |= kPqErrPlace;
                } else {
                    const uint8_t* bytes = (const uint8_t*)words;
                    for (uint64_t b = lane; k0 + b < k1; b += 64) vals[k0 + b] = bytes[b];
                }
            }
            pqw_wave_lds_order();
        } else {
            uint64_t run_at = pl.byte_base;  // the tile's bytes so far, from the page's first value byte
            for (uint32_t s = 0; s < steps; ++s) {
                const uint64_t r = r0 + 64 * s + lane;
                pqw_step(a, pc.c, r, s, levels, room, lane, live);
                uint64_t start = 0, cell = live ? row_cell(pc.c, r, start, bad) : 0;
                if (cell >= pq::kMaxCell) bad |= kPqErrCell, cell = 0, live = false;
                const uint64_t len = live ? 4 + cell : 0;
                uint64_t incl = len;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint64_t below = (uint64_t)__shfl_up((long long)incl, off, 64);
                    if ((int)lane >= off) incl += below;
                }
                const uint64_t total = (uint64_t)__shfl((long long)incl, 63, 64);
                if (run_at + total > pg.values_bytes) {  // uniform: never a store outside the page's values
                    bad |= kPqErrPlace;
                    break;
                }
                const uint64_t at = run_at + incl - len;
                run_at += total;
                // 1. The cells below kPqLongCell bytes, run by run through LDS. A run is the neighbouring rows, from
                // the first one not yet written on, whose span still fits; a longer cell ends a run.
                const bool is_long = len >= kPqLongCell;
                unsigned long long todo = __ballot(!is_long);
                while (todo) {  // uniform in the wave
                    const int first = __builtin_ctzll(todo);
                    const uint64_t lo = (uint64_t)__shfl((long long)at, first, 64);
                    const bool fits = !is_long && (int)lane >= first && at + len - lo <= kPqSpanLds;  // lane `first` always does
                    const unsigned long long gaps = ~__ballot(fits) & (~0ull << first);
                    const int stop = gaps ? __builtin_ctzll(gaps) : 64;  // the first lane behind the run
                    const unsigned long long run = (stop == 64 ? ~0ull : (1ull << stop) - 1) & (~0ull << first);
                    const bool mine = (run >> lane) & 1;
                    const uint64_t hi = (uint64_t)__shfl((long long)(at + len), stop - 1, 64);
                    const uint32_t shift = (uint32_t)((uintptr_t)(vals + lo) & 15);
                    if (mine && len) {
                        uint8_t* p = stage + shift + (uint32_t)(at - lo);
                        const uint32_t n = (uint32_t)cell;
                        __builtin_memcpy(p, &n, 4);
                        copy_span_lane(p + 4, pc.c.values + start, n);
                    }
                    pqw_wave_lds_order();  // the run is assembled
                    if (hi > lo && hi - lo <= kPqSpanLds) pqw_store_span(vals + lo, hi - lo, stage, lane);
                    pqw_wave_lds_order();  // the run is stored: the next one may overwrite it
                    todo &= ~run;
                }
                // 2. The longer cells, by the whole wave straight to the output.
                todo = __ballot(is_long);
                while (todo) {  // uniform in the wave
                    const int src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const uint64_t n = (uint64_t)__shfl((long long)cell, src, 64);
                    const uint8_t* p = pc.c.values + (uint64_t)__shfl((long long)start, src, 64);
                    uint8_t* d = vals + (uint64_t)__shfl((long long)at, src, 64);
                    if (lane < 4) d[lane] = (uint8_t)(n >> (8 * lane));
                    copy_span_wave(d + 4, p, n, lane);
                }
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kPqErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// OXH_PARQUET_SNAPPY: page k's PageHeader, heads[k].len bytes from blob[heads[k].src ..), to out[heads[k].at ..); a
// wave a page. The compressed bodies behind them are snappy_pack_kernel's.
struct PqHead {
    uint64_t at;
    uint32_t src, len;
};
__global__ __launch_bounds__(64) void pqw_heads_kernel(const PqHead* __restrict__ heads, uint64_t npages, const uint8_t* __restrict__ blob, uint8_t* out) {
    for (uint64_t k = blockIdx.x; k < npages; k += gridDim.x) copy_span_wave(out + heads[k].at, blob + heads[k].src, heads[k].len, threadIdx.x);
}

}  // namespace oxh

namespace {

using oxh::cols::is_bytes;

uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// One call over device-resident columns, in two steps: measure() knows the file's bytes and the stats (the tile
// table has come down and the plan is made), emit() sends the plan up and writes the file. The lease -- the control
// words and column table, the tile table, then the plan's places, pages and heads, sized for a page per tile -- and
// its pinned mirror live as long as the call.
struct WriteCall {
    explicit WriteCall(hipStream_t stream) : st(stream), lease(stream) {}
    ~WriteCall() {
        (void)hipStreamSynchronize(st);
        if (d_image) (void)hipFree(d_image);
    }
    hipStream_t st;
    oxh::ScratchLease lease;
    oxh::PqArgs args{};
    pq::Plan plan;
    uint8_t *d_base = nullptr, *h_base = nullptr;
    uint64_t plan_at = 0, plan_room = 0;
    unsigned long long *d_ctrl = nullptr, *h_ctrl = nullptr;

    unsigned grid() const { return (unsigned)std::min<uint64_t>((args.ntiles * args.ncols + 3) / 4, oxh::kPqMaxGroups); }
    int measure(const pq::Args& a, const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                const uint64_t* bits, const uint8_t* const* d_child, const uint64_t* child_bits, const uint64_t* elem_lo);
    int emit(uint8_t* d_out);
    // OXH_PARQUET_SNAPPY, after measure(): compress() emits the uncompressed file into an image the call owns,
    // compresses every page body -- one raw Snappy block each, snappy_compress.hip -- into the fragments' slots and
    // re-plans with the streams' sizes: `stored` is the SNAPPY file's plan, stored.out_bytes its size. pack() then
    // writes that file to d_out, every byte once: the headers (pqw_heads_kernel), the bodies (snappy_pack_kernel),
    // the magic and the footer.
    pq::Args a{};
    const pq::Tile* tiles = nullptr;
    pq::Plan stored;
    uint8_t* d_image = nullptr;  // [the image | the page tables | the Snappy working memory]
    uint64_t at_tab = 0, at_sizes = 0, at_status = 0, at_heads = 0, at_blob = 0, nfrags = 0;
    int compress();
    int pack(uint8_t* d_out);
    // OXH_PARQUET_DICTIONARY: the chunks' distinct values are built behind the measure kernel (parquet_dict.hip), what
    // the planner reads of them comes down with the tile table, and emit() writes the dictionary chunks' values
    // behind the emit kernel. The working memory lies in the lease behind the plan; it has no pinned mirror.
    oxh::PqDict dict;
    const pq::ChunkDict* dicts = nullptr;
    // List columns (parquet_write_lists.hip): their tiles are counted behind the measure kernel, their pages written
    // behind the emit kernel, in working memory of their own.
    oxh::PqLists lists;
};

int column_error(unsigned long long e) {
    if (e & oxh::kRowErrOffsets) return fail(OXH_ERR_INVALID, "parquet write: a byte column's offsets decrease or are negative");
    if (e & oxh::kRowErrValues) return fail(OXH_ERR_INVALID, "parquet write: a byte column has bytes but no values");
    if (e & oxh::kPqErrCell) return fail(OXH_ERR_INVALID, "parquet write: a string cell has 2^32 bytes or more");
    if (e & oxh::kPqErrListOffsets) return fail(OXH_ERR_INVALID, "parquet write: a list column's offsets decrease or are negative");
    if (e & oxh::kPqErrListValues) return fail(OXH_ERR_INVALID, "parquet write: a list column has elements but no values");
    if (e & oxh::kPqErrListLong) return fail(OXH_ERR_INVALID, "parquet write: a list has more than INT32_MAX elements, more than a page's int32 holds");
    if (e) return fail(OXH_ERR_HIP, "parquet write: a tile's values are not what was measured (did the columns change during the call?)");
    return OXH_OK;
}

int WriteCall::measure(const pq::Args& a, const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                       const uint64_t* bits, const uint8_t* const* d_child, const uint64_t* child_bits, const uint64_t* elem_lo) {
    const uint64_t n = a.nrows, ntiles = (n + pq::kTileRows - 1) / pq::kTileRows, items = ntiles * a.ncols;
    this->a = a;
    tiles = nullptr;
    if (n) {
        // [ctrl | columns] [tiles] [places | pages | heads]
        const uint64_t cols_at = oxh::kPqCtrlWords * 8, small = align256(cols_at + a.ncols * sizeof(oxh::PqCol));
        const uint64_t tiles_at = small;
        plan_at = tiles_at + align256(items * sizeof(pq::Tile));
        plan_room = align256(items * (sizeof(pq::Place) + sizeof(pq::Page) + 64));  // a head is below 64 bytes
        // with dictionaries: the chunks' table behind the tiles, a dictionary page and its head more per chunk
        const bool with_dict = a.flags & pq::kFlagDictionary;
        const uint64_t group_rows = pq::group_rows_of(a.rows_per_group), nchunks = (n + group_rows - 1) / group_rows * a.ncols;
        const uint64_t chunks_at = plan_at;
        if (with_dict) plan_at += align256(nchunks * sizeof(pq::ChunkDict)), plan_room += align256(nchunks * (sizeof(pq::Page) + 64));
        const uint64_t front = plan_at + plan_room, work = with_dict ? oxh::PqDict::work_bytes(n, a.ncols, a.types, group_rows) : 0;
        const uint64_t total = front + work;
        void *lbase = nullptr, *pinned = nullptr;
        if (lease.get(total, &lbase) != hipSuccess || lease.pinned(front, &pinned) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "parquet write: " + std::to_string(total) + " B of tile table, plan and dictionary tables");
        }
        d_base = (uint8_t*)lbase, h_base = (uint8_t*)pinned;
        memset(h_base, 0, cols_at);
        oxh::PqCol* h_cols = (oxh::PqCol*)(h_base + cols_at);
        for (uint32_t c = 0; c < a.ncols; ++c) {
            h_cols[c].c.values = (const uint8_t*)d_values[c];
            h_cols[c].c.offsets = is_bytes(a.kinds[c]) || pq::is_list(a.types[c]) ? (const uint8_t*)d_offsets[c] : nullptr;
            h_cols[c].c.validity = d_validity[c];
            h_cols[c].c.vbit = bits[2 * c], h_cols[c].c.nbit = bits[2 * c + 1];
            h_cols[c].c.kind = a.kinds[c], h_cols[c].c.order = 0;
            h_cols[c].type = a.types[c], h_cols[c].pad = 0;
        }
        h_ctrl = (unsigned long long*)h_base, d_ctrl = (unsigned long long*)d_base;
        args = oxh::PqArgs{(const oxh::PqCol*)(d_base + cols_at), n, ntiles, a.ncols};
        HIP_TRY(hipMemcpyAsync(d_base, h_base, small, hipMemcpyHostToDevice, st));
        oxh::pqw_measure_kernel<<<grid(), 256, 0, st>>>(args, (pq::Tile*)(d_base + tiles_at), d_ctrl);
        HIP_TRY(hipGetLastError());
        {
            const int rc = lists.measure(args, a.types, h_cols, d_child, child_bits, elem_lo, (pq::Tile*)(d_base + tiles_at), d_ctrl, h_ctrl, st);
            if (rc) return rc;
        }
        if (work) {
            const int rc = dict.build(args, a.types, group_rows, d_base + front, (pq::ChunkDict*)(d_base + chunks_at), d_ctrl, st);
            if (rc) return rc;
            dicts = (const pq::ChunkDict*)(h_base + chunks_at);
        }
        HIP_TRY(hipMemcpyAsync(h_base + tiles_at, d_base + tiles_at, (work ? plan_at - tiles_at : items * sizeof(pq::Tile)), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int rc = column_error(h_ctrl[oxh::kPqErr]);
        if (rc) return rc;
        tiles = (const pq::Tile*)(h_base + tiles_at);
    }
    static const pq::Tile none{};
    if (!tiles) tiles = &none;  // never read: there is no tile
    plan = pq::make_plan(n, a.ncols, a.types, a.names, a.name_offsets, a.rows_per_group, a.page_bytes, tiles, nullptr, dicts);
    if (!plan.error.empty()) return fail(OXH_ERR_INVALID, "parquet write: " + plan.error);
    STEP("parquet write: %llu rows x %u columns, %llu B, %llu row groups, %llu pages", (unsigned long long)n, a.ncols,
         (unsigned long long)plan.out_bytes, (unsigned long long)plan.row_groups, (unsigned long long)plan.pages.size());
    return OXH_OK;
}

// The whole file to d_out (plan.out_bytes of device memory); complete on return.
int WriteCall::emit(uint8_t* d_out) {
    HIP_TRY(hipMemcpyAsync(d_out, "PAR1", 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_out + plan.out_bytes - plan.footer.size(), plan.footer.data(), plan.footer.size(), hipMemcpyHostToDevice, st));
    if (args.nrows) {
        const uint64_t places_bytes = plan.places.size() * sizeof(pq::Place), pages_bytes = plan.pages.size() * sizeof(pq::Page);
        const uint64_t used = places_bytes + pages_bytes + plan.blob.size();
        if (used > plan_room) return fail(OXH_ERR_HIP, "parquet write: the plan outgrew its room");
        uint8_t* h = h_base + plan_at;
        memcpy(h, plan.places.data(), places_bytes);
        memcpy(h + places_bytes, plan.pages.data(), pages_bytes);
        memcpy(h + places_bytes + pages_bytes, plan.blob.data(), plan.blob.size());
        HIP_TRY(hipMemcpyAsync(d_base + plan_at, h, used, hipMemcpyHostToDevice, st));
        const uint8_t* d = d_base + plan_at;
        const oxh::PqEmit em{(const pq::Page*)(d + places_bytes), (const pq::Place*)d, d + places_bytes + pages_bytes, plan.pages.size(), d_out};
        oxh::pqw_emit_kernel<<<grid(), 256, 0, st>>>(args, em, d_ctrl);
        HIP_TRY(hipGetLastError());
        if (dicts) {
            const int rc = dict.write(args, em, plan, d_ctrl, st);
            if (rc) return rc;
        }
        const int rc = lists.emit(em, plan, d_ctrl, st);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (args.nrows && h_ctrl[oxh::kPqErr]) return column_error(h_ctrl[oxh::kPqErr]);
    return OXH_OK;
}

int WriteCall::compress() {
    const uint64_t np = plan.pages.size();
    if (!np) return stored = plan, OXH_OK;  // no page: the file is the magic and the footer
    std::vector<uint64_t> tab(2 * np), frag0(np + 1), kept(np);
    std::vector<uint32_t> frag_block, frag_size;
    for (uint64_t k = 0; k < np; ++k) {
        const pq::Page& pg = plan.pages[k];
        tab[k] = pg.file_at + plan.header_len[k], tab[np + k] = pg.file_at + pg.head_len + pg.level_bytes + pg.values_bytes;
        frag0[k] = frag_block.size();
        frag_block.insert(frag_block.end(), oxh::snappy_fragments(tab[np + k] - tab[k]), (uint32_t)k);
    }
    frag0[np] = nfrags = frag_block.size();
    frag_size.resize(nfrags);
    const uint64_t up16 = 15;
    at_tab = (plan.out_bytes + up16) & ~up16, at_sizes = at_tab + 4 * np * 8, at_status = at_sizes + np * 8;
    at_heads = (at_status + np * 4 + up16) & ~up16, at_blob = at_heads + np * sizeof(oxh::PqHead);
    const oxh::SnappyLayout lay(at_blob + np * 64, np, nfrags);  // a PageHeader is below 64 bytes
    if (hipMalloc(&d_image, lay.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet write: " + std::to_string(lay.total) + " B for the uncompressed image and the Snappy fragments");
    }
    oxh::poison_device(d_image, lay.total, st);
    int rc = emit(d_image);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_image + at_tab, tab.data(), 2 * np * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_image + lay.at_frag0, frag0.data(), (np + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_image + lay.at_block, frag_block.data(), nfrags * 4, hipMemcpyHostToDevice, st));
    const uint64_t* d_lo = (const uint64_t*)(d_image + at_tab);
    if ((rc = oxh::snappy_fragments_enqueue(d_image, d_lo, d_lo + np, lay.work(d_image, nfrags), st))) return rc;
    unsigned long long ctrl = 0;
    HIP_TRY(hipMemcpyAsync(frag_size.data(), d_image + lay.at_size, nfrags * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ctrl, d_image + lay.at_ctrl, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctrl) return fail(OXH_ERR_HIP, "parquet write: a page's Snappy fragment passed its slot");
    for (uint64_t k = 0; k < np; ++k) {
        kept[k] = pq::varint_len(tab[np + k] - tab[k]);
        for (uint64_t f = frag0[k]; f < frag0[k + 1]; ++f) kept[k] += frag_size[f];
    }
    stored = pq::make_plan(a.nrows, a.ncols, a.types, a.names, a.name_offsets, a.rows_per_group, a.page_bytes, tiles, kept.data(), dicts);
    if (!stored.error.empty()) return fail(OXH_ERR_INVALID, "parquet write: " + stored.error);
    if (stored.pages.size() != np) return fail(OXH_ERR_HIP, "parquet write: the SNAPPY plan has other pages than the uncompressed one");
    return OXH_OK;
}

int WriteCall::pack(uint8_t* d_out) {
    const uint64_t np = plan.pages.size();
    if (!np) return emit(d_out);
    std::vector<uint64_t> tab(2 * np);
    std::vector<oxh::PqHead> heads(np);
    std::vector<uint8_t> blob;
    std::vector<uint32_t> status(np);
    for (uint64_t k = 0; k < np; ++k) {
        const pq::Page& pg = stored.pages[k];
        const uint32_t len = stored.header_len[k];
        heads[k] = oxh::PqHead{pg.file_at, (uint32_t)blob.size(), len};
        blob.insert(blob.end(), stored.blob.begin() + pg.head_src, stored.blob.begin() + pg.head_src + len);
        tab[k] = pg.file_at + len, tab[np + k] = pg.file_at + len + pg.values_bytes;
    }
    if (blob.size() > np * 64) return fail(OXH_ERR_HIP, "parquet write: the page headers outgrew their room");
    const oxh::SnappyLayout lay(at_blob + np * 64, np, nfrags);
    HIP_TRY(hipMemcpyAsync(d_out, "PAR1", 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_out + stored.out_bytes - stored.footer.size(), stored.footer.data(), stored.footer.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_image + at_tab + 2 * np * 8, tab.data(), 2 * np * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_image + at_heads, heads.data(), np * sizeof(oxh::PqHead), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_image + at_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    const uint64_t* d_lo = (const uint64_t*)(d_image + at_tab);
    int rc = oxh::snappy_pack_enqueue(d_lo, d_lo + np, d_out, d_lo + 2 * np, d_lo + 3 * np, (uint64_t*)(d_image + at_sizes),
                                      (uint32_t*)(d_image + at_status), np, false, lay.work(d_image, nfrags), st);
    if (rc) return rc;
    oxh::pqw_heads_kernel<<<(unsigned)std::min<uint64_t>(np, oxh::kPqMaxGroups), 64, 0, st>>>((const oxh::PqHead*)(d_image + at_heads), np, d_image + at_blob, d_out);
    HIP_TRY(hipGetLastError());
    unsigned long long ctrl = 0;
    HIP_TRY(hipMemcpyAsync(status.data(), d_image + at_status, np * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ctrl, d_image + lay.at_ctrl, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctrl || std::any_of(status.begin(), status.end(), [](uint32_t s) { return s != 0; }))
        return fail(OXH_ERR_HIP, "parquet write: a page's Snappy stream is not what was planned");
    return OXH_OK;
}

void report(const pq::Args& a, const WriteCall& call, uint64_t bytes) {
    *a.out_bytes = bytes;
    a.stats4[0] = bytes, a.stats4[1] = call.plan.row_groups;
    a.stats4[2] = call.plan.pages.size(), a.stats4[3] = call.plan.null_cells;
}

int too_small(const pq::Args& a, uint64_t need) {
    return fail(OXH_ERR_INVALID, "parquet write: out holds " + std::to_string(a.capacity) + " B, the file has " + std::to_string(need));
}

}  // namespace

extern "C" {

int oxh_write_parquet_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                             const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                             const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint64_t rows_per_group,
                             uint64_t page_bytes, uint32_t flags, uint8_t* d_out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4,
                             void* stream) {
    return oxh_write_parquet_lists_device(ctx, nrows, ncols, types, kinds, d_values, d_offsets, d_validity, bit_offsets, names, name_offsets,
                                          rows_per_group, page_bytes, flags, d_out, capacity, out_bytes, stats4, stream, nullptr, nullptr);
}

int oxh_write_parquet_lists_device(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                                   const void* const* d_values, const void* const* d_offsets, const uint8_t* const* d_validity,
                                   const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint64_t rows_per_group,
                                   uint64_t page_bytes, uint32_t flags, uint8_t* d_out, uint64_t capacity, uint64_t* out_bytes,
                                   uint64_t* stats4, void* stream, const uint8_t* const* d_child_validity, const uint64_t* child_bit_offsets) {
    const pq::Args a{nrows, ncols, types, kinds, d_values, d_offsets, d_validity, bit_offsets, names, name_offsets,
                     rows_per_group, page_bytes, flags, d_out, capacity, out_bytes, stats4, d_child_validity, child_bit_offsets};
    const std::string what = pq::write_error(a, false);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet write: " + what);
    int rc = device_enter(ctx);
    if (rc) return rc;
    WriteCall call((hipStream_t)stream);
    if ((rc = call.measure(a, d_values, d_offsets, d_validity, bit_offsets, d_child_validity, child_bit_offsets, nullptr))) return rc;
    const bool snappy = flags & pq::kFlagSnappy;
    // with the flag the size is known only after compressing: `need` is a capacity that always suffices
    const uint64_t need = snappy ? pq::snappy_capacity(call.plan, ncols) : call.plan.out_bytes;
    if (d_out && capacity >= need && (rc = snappy ? call.compress() : call.emit(d_out))) return rc;
    if (snappy && d_out && capacity >= need) {
        if (call.stored.out_bytes > capacity) return fail(OXH_ERR_HIP, "parquet write: the SNAPPY file passed its bound");
        if ((rc = call.pack(d_out))) return rc;
        report(a, call, call.stored.out_bytes);
        return OXH_OK;
    }
    report(a, call, need);
    return d_out && capacity < need ? too_small(a, need) : OXH_OK;
}

int oxh_write_parquet_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                           const void* const* values, const void* const* offsets, const uint8_t* const* validity,
                           const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint64_t rows_per_group,
                           uint64_t page_bytes, uint32_t flags, uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4) {
    return oxh_write_parquet_lists_host(ctx, nrows, ncols, types, kinds, values, offsets, validity, bit_offsets, names, name_offsets, rows_per_group,
                                        page_bytes, flags, out, capacity, out_bytes, stats4, nullptr, nullptr);
}

int oxh_write_parquet_lists_host(oxh_ctx* ctx, uint64_t nrows, uint32_t ncols, const uint32_t* types, const uint32_t* kinds,
                                 const void* const* values, const void* const* offsets, const uint8_t* const* validity,
                                 const uint64_t* bit_offsets, const uint8_t* names, const uint64_t* name_offsets, uint64_t rows_per_group,
                                 uint64_t page_bytes, uint32_t flags, uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* stats4,
                                 const uint8_t* const* child_validity, const uint64_t* child_bit_offsets) {
    const pq::Args a{nrows, ncols, types, kinds, values, offsets, validity, bit_offsets, names, name_offsets,
                     rows_per_group, page_bytes, flags, out, capacity, out_bytes, stats4, child_validity, child_bit_offsets};
    const std::string what = pq::write_error(a, true);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "parquet write: " + what);
    int rc = device_enter(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    // One device block for the inputs: of every column only what its rows name (columns.hpp).
    oxh::cols::Staging staging;
    std::vector<oxh::cols::Staged> staged(ncols);
    // a list column: its offsets, its lists' bitmap, and of its elements and their bitmap the span [lo, hi) that the
    // lists which are not null name -- the kernels subtract lo (elem_lo) from an element's index
    std::vector<int64_t> child_piece(ncols, -1);
    std::vector<uint64_t> child_bits(ncols, 0), elem_lo(ncols, 0);
    for (uint32_t c = 0; c < ncols && nrows; ++c) {
        if (!pq::is_list(types[c])) {
            staged[c] = staging.add_column(kinds[c], values[c], offsets[c], validity[c], bit_offsets[2 * c], bit_offsets[2 * c + 1], nrows);
            continue;
        }
        const pq::ListSpan span = pq::list_span(a, c);
        const uint32_t w = pq::element_width(types[c]);
        elem_lo[c] = span.lo;
        staged[c].offsets = staging.add(offsets[c], (nrows + 1) * pq::list_offset_width(types[c]));
        if (span.hi > span.lo) staged[c].values = staging.add((const uint8_t*)values[c] + w * span.lo, w * (span.hi - span.lo));
        if (validity[c]) staged[c].validity = staging.add_bits(validity[c], bit_offsets[2 * c + 1], nrows, staged[c].nbit);
        if (child_validity && child_validity[c] && span.hi > span.lo)
            child_piece[c] = staging.add_bits(child_validity[c], (child_bit_offsets ? child_bit_offsets[c] : 0) + span.lo, span.hi - span.lo, child_bits[c]);
    }
    uint8_t *d_in = nullptr, *d_out = nullptr;
    if (staging.total && hipMalloc(&d_in, staging.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "parquet write: " + std::to_string(staging.total) + " B for the columns on the device");
    }
    oxh::poison_device(d_in, staging.total, st);
    uint64_t need = 0;
    bool fits = false;
    rc = [&]() -> int {
        for (const oxh::cols::Piece& p : staging.pieces)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(d_in + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
        std::vector<const void*> d_values(ncols, nullptr), d_offsets(ncols, nullptr);
        std::vector<const uint8_t*> d_validity(ncols, nullptr), d_child(ncols, nullptr);
        std::vector<uint64_t> bits(2 * (size_t)ncols, 0);
        for (uint32_t c = 0; c < ncols && nrows; ++c) {
            d_values[c] = staging.values_at(d_in, staged[c]);
            d_offsets[c] = staging.offsets_at(d_in, staged[c]);
            d_validity[c] = staging.validity_at(d_in, staged[c]);
            bits[2 * c] = staged[c].vbit, bits[2 * c + 1] = staged[c].nbit;
            if (child_piece[c] >= 0) d_child[c] = d_in + staging.pieces[child_piece[c]].at;
        }
        WriteCall call(st);
        int r = call.measure(a, d_values.data(), d_offsets.data(), d_validity.data(), bits.data(), d_child.data(), child_bits.data(), elem_lo.data());
        if (r) return r;
        const bool snappy = flags & pq::kFlagSnappy;
        need = snappy ? pq::snappy_capacity(call.plan, ncols) : call.plan.out_bytes;
        fits = out && capacity >= need;
        uint64_t bytes = need;
        if (fits) {
            if (snappy) {
                if ((r = call.compress())) return r;
                if ((bytes = call.stored.out_bytes) > capacity) return fail(OXH_ERR_HIP, "parquet write: the SNAPPY file passed its bound");
            }
            if (hipMalloc(&d_out, bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(OXH_ERR_NOMEM, "parquet write: " + std::to_string(bytes) + " B for the file on the device");
            }
            oxh::poison_device(d_out, bytes, st);
            if ((r = snappy ? call.pack(d_out) : call.emit(d_out))) return r;
            HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        report(a, call, bytes);
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (rc) return rc;
    return out && !fits ? too_small(a, need) : OXH_OK;
}

}  // extern "C"
