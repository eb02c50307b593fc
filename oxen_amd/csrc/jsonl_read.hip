// oxen_amd/csrc/jsonl_read.hip -- JSON Lines bytes in HBM to a record index and to typed Arrow columns
// (oxh_jsonl_*): the `"ndjson" | "jsonl"` arm of the reference's readers (core/df/tabular.rs:73-82 read_df_jsonl).
// The rules are stated in include/oxen_hash.h "JSON Lines"; the cell grammar, the unescape step, the key compare
// and the carries are jsonl_text.hpp's, the code tests/native/jsonl_host_test.cpp runs on the host; the checks and
// the sizes are jsonl_host.hpp's; the column entries' checks, sizes and deferred floats are csv_host.hpp's.
//
// Three states restart at every '\n': the run of backslashes, the string parity and the depth. Each is a value
// with an associative compose (jsonl_text.hpp), folded over a lane's 16 bytes by bit operations, over a wave by
// shuffles, over a workgroup's 4 KiB tile through LDS, and over the tiles by one workgroup that walks their
// per-tile values in order. A unit that is all backslashes has even length and passes the carry through.
//
// The index (oxh_jsonl_open_*), on one stream; every kernel over the bytes has csv_read.hip's shape (a lane loads
// 16 bytes of the 16-byte aligned space around d_bytes, bytewise at the head and the tail; grid-stride tiles):
//   escapes   jsonl_esc_kernel: per tile its backslash carry; jsonl_esc_carry_kernel: the carry into every tile;
//   lines     jsonl_line_kernel: the escaped bytes, so the unescaped quotes; per tile its line carry (holds a
//             '\n'; the parity and the depth change, entered outside or inside a string); jsonl_line_carry_kernel:
//             the (inside a string, depth) every tile is entered with;
//   count     jsonl_kept_kernel<false>: per tile the kept bytes -- the openers that leave depth 0, the closers that
//             reach it, the ':' and ',' at depth 1, all outside strings, and every '\n' -- and the line ends. The
//             position one past the last byte ends the last line unless the last byte did;
//   scan x 2, then jsonl_kept_kernel<true>: ends[] = the kept positions, ascending; rec_end[] = for every line the
//             place of its end in ends[]: a CSR of lines over the kept bytes, as the CSV reader's;
//   row map   jsonl_keep_kernel (a line is blank: no kept byte and whitespace only), the scan, jsonl_rowmap_kernel:
//             row_rec[] = the records; jsonl_wellformed_kernel: a bit per record, the first well-formed one;
//   schema    the keys of the first well-formed record come down; jsonl_canon_kernel marks the canonical rows (the
//             keys are the first k names in order) and lists the others inside the window; only their keys come
//             down (jsonl_keys_len_kernel, two scans, jsonl_keys_copy_kernel), the host appends the unseen ones,
//             and where the names grew jsonl_canon_kernel runs once more for the counts against all names.
// The columns (oxh_jsonl_columns_*), one lane per row, 64 rows per wave, as the CSV reader's: a canonical row reads
// field c, any other searches its keys from the front. A string cell of kLongCell bytes and more without an
// escape is looked through and copied by the whole wave; one WITH an escape is walked and unescaped by its own lane
// (exact, serial: not the CSV reader's whole-wave unescape). No workgroup ever waits for another; launches order the steps. A place from
// a scan is checked before it is stored through: a bad one sets the error word (OXH_ERR_HIP).
#include "capi_internal.hpp"
#include "columns.hpp"
#include "jsonl_host.hpp"

using namespace oxh::capi;

namespace oxh {

__constant__ double kJsonlPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                       1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

constexpr uint32_t kJlTileBytes = csv::kTileBytes;
constexpr uint32_t kJlLongCell = csv::kLongCell;
constexpr uint32_t kJlDeferSlot = csv::kDeferSlot;
constexpr unsigned long long kJlErrPlace = 4;
// ctrl words of an open: the error word, the malformed records, the first well-formed row (+ 1; 0: none), the
// non-canonical rows, the ignored fields, the nested values
constexpr int kJlCtrlErr = 0, kJlCtrlMalformed = 1, kJlCtrlFirst = 2, kJlCtrlNonCanon = 3, kJlCtrlIgnored = 4, kJlCtrlNested = 5,
              kJlCtrlWords = 8;
// ctrl words of one selected column: stats4's first three, the string bytes, the error word
constexpr int kJlColEmpty = 0, kJlColBad = 1, kJlColDeferred = 2, kJlColBytes = 3, kJlColErr = 4, kJlColWords = 8;

// What the row kernels read of a handle.
struct JsonlView {
    const uint8_t* bytes;
    const uint32_t* ends;
    const uint32_t* rec_end;
    const uint32_t* row_rec;
    const uint64_t* wf;     // bit per row: the record is well formed
    const uint64_t* canon;  // bit per row: its keys are the first k names in order
    const uint8_t* names;
    const uint32_t* name_offsets;
    uint64_t nrows;
    uint32_t ncols;
};

struct JsonlCell {
    const uint8_t* p;  // the trimmed value slot
    uint32_t n;
    bool present;
};

// Line r: its bytes [a, b) and its m kept positions s[0 .. m).
__device__ __forceinline__ void jsonl_line(const uint32_t* ends, const uint32_t* rec_end, uint32_t r, uint32_t& a, uint32_t& b, const uint32_t*& s,
                                           uint32_t& m) {
    const uint32_t first = r ? rec_end[r - 1] + 1 : 0, term = rec_end[r];
    a = first ? ends[first - 1] + 1 : 0, b = ends[term];
    s = ends + first, m = term - first;
}

__device__ __forceinline__ bool jsonl_bit(const uint64_t* words, uint64_t i) { return (words[i >> 6] >> (i & 63)) & 1; }

__device__ __forceinline__ JsonlCell jsonl_cell(const JsonlView& v, uint64_t row, uint32_t col) {
    JsonlCell c{nullptr, 0, false};
    if (!jsonl_bit(v.wf, row)) return c;
    uint32_t a, b, m;
    const uint32_t* s;
    jsonl_line(v.ends, v.rec_end, v.row_rec[row], a, b, s, m);
    const uint32_t k = jsonl::record_fields(m);
    if (jsonl_bit(v.canon, row)) {
        if (col >= k) return c;
        jsonl::value_slot(v.bytes, s, col, c.p, c.n);
        c.present = true;
        return c;
    }
    const uint8_t* name = v.names + v.name_offsets[col];
    const uint32_t len = v.name_offsets[col + 1] - v.name_offsets[col];
    for (uint32_t f = 0; f < k; ++f) {  // the first occurrence wins
        const uint8_t* kp;
        uint32_t kn;
        jsonl::key_slot(v.bytes, s, f, kp, kn);
        if (!jsonl::key_equals(kp, kn, name, len)) continue;
        jsonl::value_slot(v.bytes, s, f, c.p, c.n);
        c.present = true;
        return c;
    }
    return c;
}

// ---------------------------------------------------------------- folds over a workgroup
template <class T>
__device__ __forceinline__ T jsonl_shfl_up(T v, int off) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / 4; ++k) w[k] = (uint32_t)__shfl_up((int)w[k], off, 64);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
}

struct JsonlSum {
    uint32_t v;
    static __device__ __forceinline__ JsonlSum identity() { return JsonlSum{0}; }
    static __device__ __forceinline__ JsonlSum compose(JsonlSum a, JsonlSum b) { return JsonlSum{a.v + b.v}; }
};

// The fold of the values of the lanes before this one, in lane order over the 256 lanes, and of all of them.
// part: 4 T of LDS. Every lane of the workgroup calls it.
template <class T>
__device__ __forceinline__ T jsonl_block_exclusive(T mine, T* part, T& total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = jsonl_shfl_up(incl, off);
        if (lane >= (unsigned)off) incl = T::compose(up, incl);
    }
    const T prev = jsonl_shfl_up(incl, 1);
    __syncthreads();  // the parts of the call before have been read
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    T before = T::identity();
    for (unsigned w = 0; w < wave; ++w) before = T::compose(before, part[w]);
    total = T::compose(T::compose(part[0], part[1]), T::compose(part[2], part[3]));
    return lane ? T::compose(before, prev) : before;
}

// One workgroup over the per-tile values in order: store(t, the fold of the tiles before t). A lane folds
// kCarryChunk tiles one after the other, the workgroup 256 such chunks a round.
template <class T, class Load, class Store>
__device__ __forceinline__ void jsonl_carry_scan(uint64_t ntiles, Load load, Store store, T* part) {
    T running = T::identity();  // the same in every lane
    for (uint64_t base = 0; base < ntiles; base += 256ull * jsonl::kCarryChunk) {  // uniform in the workgroup
        const uint64_t first = base + (uint64_t)threadIdx.x * jsonl::kCarryChunk;
        T v[jsonl::kCarryChunk];
        T mine = T::identity();
#pragma unroll
        for (uint32_t k = 0; k < jsonl::kCarryChunk; ++k) {
            v[k] = first + k < ntiles ? load(first + k) : T::identity();
            mine = T::compose(mine, v[k]);
        }
        T total;
        T p = T::compose(running, jsonl_block_exclusive(mine, part, total));
#pragma unroll
        for (uint32_t k = 0; k < jsonl::kCarryChunk; ++k) {
            if (first + k < ntiles) store(first + k, p);
            p = T::compose(p, v[k]);
        }
        running = T::compose(running, total);
    }
}

// ---------------------------------------------------------------- the index
struct JsonlMasks {
    uint32_t bs, q, nl, op, cl, co;  // backslashes, quotes, newlines, { [, } ], : and ,
};

__device__ __forceinline__ void jsonl_byte_masks(uint32_t c, uint32_t at, JsonlMasks& m) {
    m.bs |= (uint32_t)(c == '\\') << at;
    m.q |= (uint32_t)(c == '"') << at;
    m.nl |= (uint32_t)(c == '\n') << at;
    m.op |= (uint32_t)((c | 0x20) == '{') << at;  // '[' | 0x20 == '{'
    m.cl |= (uint32_t)((c | 0x20) == '}') << at;  // ']' | 0x20 == '}'
    m.co |= (uint32_t)(c == ':' || c == ',') << at;
}

__device__ __forceinline__ void jsonl_word_masks(uint32_t w, uint32_t at, JsonlMasks& m) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) jsonl_byte_masks((w >> (8 * k)) & 0xFF, at + k, m);
}

// The lane's 16 bytes at v0 (a multiple of 16) of the aligned space; the buffer is [lo, hi) of it. A byte outside
// the buffer is in no mask and is never loaded.
__device__ __forceinline__ JsonlMasks jsonl_lane_masks(const uint8_t* base, uint64_t v0, uint64_t lo, uint64_t hi) {
    JsonlMasks m{0, 0, 0, 0, 0, 0};
    if (v0 >= lo && v0 + 16 <= hi) {
        const uint4 w = *(const uint4*)(base + v0);
        jsonl_word_masks(w.x, 0, m);
        jsonl_word_masks(w.y, 4, m);
        jsonl_word_masks(w.z, 8, m);
        jsonl_word_masks(w.w, 12, m);
    } else if (v0 + 16 > lo && v0 < hi) {
        for (uint32_t j = 0; j < 16; ++j) {
            const uint64_t at = v0 + j;
            if (at < lo || at >= hi) continue;
            jsonl_byte_masks(base[at], j, m);
        }
    }
    return m;
}

__global__ __launch_bounds__(256) void jsonl_esc_kernel(const uint8_t* __restrict__ base, uint64_t lo, uint64_t hi, uint64_t ntiles,
                                                        uint32_t* __restrict__ tile_esc) {
    __shared__ jsonl::EscCarry part[4];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // uniform in the workgroup
        const JsonlMasks m = jsonl_lane_masks(base, t * kJlTileBytes + 16ull * threadIdx.x, lo, hi);
        jsonl::EscCarry total;
        (void)jsonl_block_exclusive(jsonl::esc_of_lane(m.bs), part, total);
        if (threadIdx.x == 0) tile_esc[t] = total.v;
    }
}

__global__ __launch_bounds__(256) void jsonl_esc_carry_kernel(const uint32_t* __restrict__ tile_esc, uint64_t ntiles, uint32_t* __restrict__ tile_esc_in) {
    __shared__ jsonl::EscCarry part[4];
    jsonl_carry_scan<jsonl::EscCarry>(
        ntiles, [&](uint64_t t) { return jsonl::EscCarry{tile_esc[t]}; },
        [&](uint64_t t, jsonl::EscCarry p) { tile_esc_in[t] = jsonl::esc_in(p, 0); }, part);
}

// The lane's unescaped quotes: the escape carry across the tile's lanes, then the escaped bytes of its 16.
__device__ __forceinline__ uint32_t jsonl_unescaped_quotes(const JsonlMasks& m, uint32_t tile_in, jsonl::EscCarry* part) {
    jsonl::EscCarry total;
    const jsonl::EscCarry before = jsonl_block_exclusive(jsonl::esc_of_lane(m.bs), part, total);
    return m.q & ~jsonl::escaped_mask(m.bs, jsonl::esc_in(before, tile_in));
}

using JsonlLine32 = jsonl::LineCarry<int32_t>;
using JsonlLine64 = jsonl::LineCarry<int64_t>;

__global__ __launch_bounds__(256) void jsonl_line_kernel(const uint8_t* __restrict__ base, uint64_t lo, uint64_t hi, uint64_t ntiles,
                                                         const uint32_t* __restrict__ tile_esc_in, uint32_t* __restrict__ tile_flags,
                                                         int32_t* __restrict__ tile_d0, int32_t* __restrict__ tile_d1) {
    __shared__ jsonl::EscCarry part_e[4];
    __shared__ JsonlLine32 part_l[4];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // uniform in the workgroup
        const JsonlMasks m = jsonl_lane_masks(base, t * kJlTileBytes + 16ull * threadIdx.x, lo, hi);
        const uint32_t uq = jsonl_unescaped_quotes(m, tile_esc_in[t], part_e);
        JsonlLine32 total;
        (void)jsonl_block_exclusive(jsonl::line_of_lane(uq, m.nl, m.op, m.cl), part_l, total);
        if (threadIdx.x == 0) tile_flags[t] = total.reset | (total.par << 1), tile_d0[t] = total.d0, tile_d1[t] = total.d1;
    }
}

__global__ __launch_bounds__(256) void jsonl_line_carry_kernel(const uint32_t* __restrict__ tile_flags, const int32_t* __restrict__ tile_d0,
                                                               const int32_t* __restrict__ tile_d1, uint64_t ntiles,
                                                               uint32_t* __restrict__ tile_par_in, int64_t* __restrict__ tile_depth_in) {
    __shared__ JsonlLine64 part[4];
    jsonl_carry_scan<JsonlLine64>(
        ntiles, [&](uint64_t t) { return JsonlLine64{tile_flags[t] & 1, (tile_flags[t] >> 1) & 1, tile_d0[t], tile_d1[t]}; },
        [&](uint64_t t, JsonlLine64 p) { tile_par_in[t] = p.par, tile_depth_in[t] = p.d0; }, part);  // the buffer starts a line
}

// EMIT false: tile_kept[t] / tile_recs[t] = the tile's kept positions / those that end a line.
// EMIT true (the two are scanned): ends[] and rec_end[].
template <bool EMIT>
__global__ __launch_bounds__(256) void jsonl_kept_kernel(const uint8_t* __restrict__ base, uint64_t lo, uint64_t hi, uint64_t ntiles,
                                                         const uint32_t* __restrict__ tile_esc_in, const uint32_t* __restrict__ tile_par_in,
                                                         const int64_t* __restrict__ tile_depth_in, uint32_t* __restrict__ tile_kept,
                                                         uint32_t* __restrict__ tile_recs, const uint64_t* __restrict__ kept_scan,
                                                         const uint64_t* __restrict__ rec_scan, uint32_t* __restrict__ ends,
                                                         uint32_t* __restrict__ rec_end, uint64_t nends, uint64_t nrec,
                                                         unsigned long long* __restrict__ ctrl) {
    __shared__ jsonl::EscCarry part_e[4];
    __shared__ JsonlLine32 part_l[4];
    __shared__ JsonlSum part_s[4];
    unsigned long long bad = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // uniform in the workgroup
        const uint64_t v0 = t * kJlTileBytes + 16ull * threadIdx.x;
        const JsonlMasks m = jsonl_lane_masks(base, v0, lo, hi);
        const uint32_t uq = jsonl_unescaped_quotes(m, tile_esc_in[t], part_e);
        JsonlLine32 ltotal;
        const JsonlLine32 before = jsonl_block_exclusive(jsonl::line_of_lane(uq, m.nl, m.op, m.cl), part_l, ltotal);
        const uint32_t par_in = tile_par_in[t];
        const uint32_t inside = before.reset ? before.par : par_in ^ before.par;
        const int64_t depth = before.reset ? (int64_t)before.d0 : tile_depth_in[t] + (par_in ? before.d1 : before.d0);
        uint32_t delim = jsonl::kept_of_lane(uq, m.nl, m.op, m.cl, m.co, inside, depth) | m.nl, rec = m.nl;
        if (hi >= v0 && hi < v0 + 16) {  // one past the last byte: ends the last line unless the last byte did
            const uint32_t j = (uint32_t)(hi - v0);
            const bool last_nl = j ? (m.nl >> (j - 1)) & 1 : base[hi - 1] == '\n';
            if (!last_nl) delim |= 1u << j, rec |= 1u << j;
        }
        // both counts in one word: a tile has at most 4 097 of either
        const JsonlSum mine{(uint32_t)__popc(delim) | ((uint32_t)__popc(rec) << 16)};
        JsonlSum stotal;
        const uint32_t sofar = jsonl_block_exclusive(mine, part_s, stotal).v;
        if (!EMIT) {
            if (threadIdx.x == 0) tile_kept[t] = stotal.v & 0xFFFF, tile_recs[t] = stotal.v >> 16;
        } else {
            uint64_t pd = kept_scan[t] + (sofar & 0xFFFF), pr = rec_scan[t] + (sofar >> 16);
            while (delim) {
                const uint32_t j = __builtin_ctz(delim);
                delim &= delim - 1;
                if (pd < nends)
                    ends[pd] = (uint32_t)(v0 + j - lo);
                else
                    bad |= kJlErrPlace;
                if ((rec >> j) & 1) {
                    if (pr < nrec)
                        rec_end[pr] = (uint32_t)pd;
                    else
                        bad |= kJlErrPlace;
                    ++pr;
                }
                ++pd;
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJlCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// mask[k] = the lines of block k (lines 64k .. 64k + 63) that are records (not blank), counts[k] = how many.
__global__ __launch_bounds__(256) void jsonl_keep_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ ends,
                                                         const uint32_t* __restrict__ rec_end, uint64_t nrec, uint64_t* __restrict__ mask,
                                                         uint32_t* __restrict__ counts) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (nrec + stride - 1) / stride;  // uniform: every lane reaches the ballot
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t r = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool kept = false;
        if (r < nrec) {
            uint32_t a, b, m;
            const uint32_t* s;
            jsonl_line(ends, rec_end, (uint32_t)r, a, b, s, m);
            kept = m != 0 || !jsonl::all_ws(bytes, a, b);
        }
        const unsigned long long word = __ballot(kept);
        if (lane == 0 && r < nrec) mask[r >> 6] = word, counts[r >> 6] = (uint32_t)__popcll(word);
    }
}

// The entries of a mask-and-scan compaction: out[place] = i for every set bit i < n; a place is at most its entry.
__global__ __launch_bounds__(256) void jsonl_rowmap_kernel(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ bases, uint64_t n,
                                                           uint32_t* __restrict__ out, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t word = mask[r >> 6];
        if (!((word >> lane) & 1)) continue;
        const uint64_t place = bases[r >> 6] + (uint64_t)__popcll(word & ((1ull << lane) - 1));
        if (place <= r)  // the set bits before r: never a store outside the n places
            out[place] = (uint32_t)r;
        else
            bad |= kJlErrPlace;
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJlCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (row_rec is written) wf[k] = the well-formed records of rows 64k .. 64k + 63; ctrl: the malformed ones, and the
// first well-formed row + 1.
__global__ __launch_bounds__(256) void jsonl_wellformed_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ ends,
                                                               const uint32_t* __restrict__ rec_end, const uint32_t* __restrict__ row_rec,
                                                               uint64_t nrows, uint64_t* __restrict__ wf, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (nrows + stride - 1) / stride;  // uniform: every lane reaches the ballot
    unsigned long long malformed = 0, first = ~0ull;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool ok = false;
        if (i < nrows) {
            uint32_t a, b, m;
            const uint32_t* s;
            jsonl_line(ends, rec_end, row_rec[i], a, b, s, m);
            ok = jsonl::record_well_formed(bytes, a, b, s, m);
        }
        const unsigned long long word = __ballot(ok);
        if (lane == 0 && i < nrows) {
            wf[i >> 6] = word;
            const uint64_t here = nrows - i < 64 ? nrows - i : 64;
            malformed += here - (uint64_t)__popcll(word);
            if (word && first == ~0ull) first = i + (uint64_t)__builtin_ctzll(word);
        }
    }
    if (lane == 0) {
        if (malformed) atomicAdd(&ctrl[kJlCtrlMalformed], malformed);
        if (first != ~0ull) atomicMax(&ctrl[kJlCtrlFirst], ~first);  // the smallest row: the largest complement
    }
}

// A row that is not canonical compares each of its keys with every name, through the decode step: fields x ncols
// per such row, on every row of the file and once more where the window grew the names. Files whose rows keep one
// key order pay nothing; a wide file of reordered rows pays that product (at most 65 535 names).
// canon[k] = the canonical rows of block k. ctrl: the well-formed rows that are not canonical, the fields whose
// key is no name, the nested values. With list_mask: list_mask[k] / list_counts[k] = the non-canonical well-formed
// rows among the first `window` rows.
__global__ __launch_bounds__(256) void jsonl_canon_kernel(const JsonlView v, uint64_t* __restrict__ canon, uint64_t window,
                                                          uint64_t* __restrict__ list_mask, uint32_t* __restrict__ list_counts,
                                                          unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = v.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    unsigned long long ignored = 0, nested = 0, noncanon = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool is_canon = false, is_wf = false;
        if (i < n && jsonl_bit(v.wf, i)) {
            is_wf = is_canon = true;
            uint32_t a, b, m;
            const uint32_t* s;
            jsonl_line(v.ends, v.rec_end, v.row_rec[i], a, b, s, m);
            const uint32_t k = jsonl::record_fields(m);
            for (uint32_t f = 0; f < k; ++f) {
                const uint8_t* p;
                uint32_t len;
                jsonl::key_slot(v.bytes, s, f, p, len);
                bool same = f < v.ncols && jsonl::key_equals(p, len, v.names + v.name_offsets[f], v.name_offsets[f + 1] - v.name_offsets[f]);
                if (!same) {
                    is_canon = false;
                    bool known = false;
                    for (uint32_t c = 0; c < v.ncols && !known; ++c)
                        known = jsonl::key_equals(p, len, v.names + v.name_offsets[c], v.name_offsets[c + 1] - v.name_offsets[c]);
                    if (!known) ++ignored;
                }
                jsonl::value_slot(v.bytes, s, f, p, len);
                if (len && (p[0] == '{' || p[0] == '[')) ++nested;
            }
        }
        const unsigned long long cword = __ballot(is_canon), lword = __ballot(is_wf && !is_canon && i < window);
        noncanon += __popcll(__ballot(is_wf && !is_canon));
        if (lane == 0 && i < n) {
            canon[i >> 6] = cword;
            if (list_mask && i < window) list_mask[i >> 6] = lword, list_counts[i >> 6] = (uint32_t)__popcll(lword);
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        ignored += (unsigned long long)__shfl_xor((long long)ignored, off, 64);
        nested += (unsigned long long)__shfl_xor((long long)nested, off, 64);
    }
    if (lane == 0) {
        if (noncanon) atomicAdd(&ctrl[kJlCtrlNonCanon], noncanon);
        if (ignored) atomicAdd(&ctrl[kJlCtrlIgnored], ignored);
        if (nested) atomicAdd(&ctrl[kJlCtrlNested], nested);
    }
}

// Per listed row (well formed): how many keys it has and the bytes of their string tokens.
__global__ __launch_bounds__(256) void jsonl_keys_len_kernel(const JsonlView v, const uint32_t* __restrict__ list, uint64_t nlist,
                                                             uint32_t* __restrict__ nkeys, uint32_t* __restrict__ key_bytes) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nlist; j += stride) {
        const uint64_t row = list[j];
        uint32_t k = 0, total = 0;
        if (row < v.nrows && jsonl_bit(v.wf, row)) {
            uint32_t a, b, m;
            const uint32_t* s;
            jsonl_line(v.ends, v.rec_end, v.row_rec[row], a, b, s, m);
            k = jsonl::record_fields(m);
            for (uint32_t f = 0; f < k; ++f) {
                const uint8_t* p;
                uint32_t len;
                jsonl::key_slot(v.bytes, s, f, p, len);
                total += len;
            }
        }
        nkeys[j] = k, key_bytes[j] = total;
    }
}

// (both are scanned) key_lens[] = the length of every key token of the listed rows, text[] = the tokens.
__global__ __launch_bounds__(256) void jsonl_keys_copy_kernel(const JsonlView v, const uint32_t* __restrict__ list, uint64_t nlist,
                                                              const uint64_t* __restrict__ nkeys_scan, const uint64_t* __restrict__ bytes_scan,
                                                              uint64_t total_keys, uint64_t total_bytes, uint32_t* __restrict__ key_lens,
                                                              uint8_t* __restrict__ text, unsigned long long* __restrict__ ctrl) {
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nlist; j += stride) {
        const uint64_t row = list[j];
        if (row >= v.nrows || !jsonl_bit(v.wf, row)) continue;
        uint32_t a, b, m;
        const uint32_t* s;
        jsonl_line(v.ends, v.rec_end, v.row_rec[row], a, b, s, m);
        const uint32_t k = jsonl::record_fields(m);
        uint64_t at_key = nkeys_scan[j], at_byte = bytes_scan[j];
        for (uint32_t f = 0; f < k; ++f) {
            const uint8_t* p;
            uint32_t len;
            jsonl::key_slot(v.bytes, s, f, p, len);
            if (at_key >= total_keys || at_byte + len > total_bytes) {
                bad |= kJlErrPlace;
                break;
            }
            key_lens[at_key++] = len;
            for (uint32_t x = 0; x < len; ++x) text[at_byte + x] = p[x];
            at_byte += len;
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJlCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- the columns
// A wave's word of 64 rows as the up to 8 bytes of an Arrow bitmap from bit 0 that lie within the n rows:
// row0 = the wave's first row (a multiple of 64).
__device__ __forceinline__ void jsonl_store_word(uint8_t* bitmap, unsigned long long word, uint64_t row0, uint64_t n, unsigned lane) {
    if (bitmap && lane < 8 && row0 + 8 * lane < n) bitmap[(row0 >> 3) + lane] = (uint8_t)(word >> (8 * lane));
}

// INT64 / FLOAT64 (values: 8 bytes per row) and BOOL (values: a bit per row). With NULL outputs: the counts only.
template <uint32_t TYPE>
__global__ __launch_bounds__(256) void jsonl_fixed_kernel(const JsonlView v, uint32_t col, uint64_t* __restrict__ values, uint8_t* __restrict__ bits,
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
            const JsonlCell c = jsonl_cell(v, i, col);
            const uint32_t kind = c.present ? jsonl::cell_kind_shallow(c.p, c.n) : jsonl::kNull;
            if (kind == jsonl::kNull) {
                empty = true;
            } else if (TYPE == OXH_CSV_INT64) {
                int64_t x = 0;
                valid = kind == jsonl::kInteger && csvnum::parse_int64(c.p, c.n, x) == csvnum::kIntValue;
                word = valid ? (uint64_t)x : 0;
            } else if (TYPE == OXH_CSV_FLOAT64) {
                if (kind == jsonl::kInteger || kind == jsonl::kNumber) {
                    uint64_t m;
                    int32_t e10;
                    bool neg;
                    const uint32_t how = csvnum::parse_float(c.p, c.n, m, e10, neg);
                    valid = how == csvnum::kFloatExact || how == csvnum::kFloatDeferred;
                    deferred = how == csvnum::kFloatDeferred;
                    if (how == csvnum::kFloatExact) word = (uint64_t)__double_as_longlong(csvnum::exact_value(m, e10, neg, kJsonlPow10));
                }
            } else {
                valid = kind == jsonl::kTrue || kind == jsonl::kFalse;
                truth = kind == jsonl::kTrue;
            }
            if (TYPE != OXH_CSV_BOOL && values) values[i] = word;
        }
        const uint64_t row0 = i - lane;
        const unsigned long long vword = __ballot(valid);
        jsonl_store_word(validity, vword, row0, n, lane);
        if (TYPE == OXH_CSV_BOOL) jsonl_store_word(bits, __ballot(truth), row0, n, lane);
        n_empty += __popcll(__ballot(empty));
        n_bad += __popcll(__ballot(i < n && !valid && !empty));
        if (TYPE == OXH_CSV_FLOAT64) {
            const unsigned long long dword = __ballot(deferred);
            n_deferred += __popcll(dword);
            if (defer_mask && lane == 0 && i < n) defer_mask[i >> 6] = dword, defer_counts[i >> 6] = (uint32_t)__popcll(dword);
        }
    }
    if (lane == 0) {
        if (n_empty) atomicAdd(&ctrl[kJlColEmpty], n_empty);
        if (n_bad) atomicAdd(&ctrl[kJlColBad], n_bad);
        if (n_deferred) atomicAdd(&ctrl[kJlColDeferred], n_deferred);
    }
}

// (the masks are written, the counts scanned) For deferred cell number `place` of the column: list[3 place ..] =
// {row, where its text starts, its length}, and the first kJlDeferSlot bytes of the text in its slot.
__global__ __launch_bounds__(256) void jsonl_defer_emit_kernel(const JsonlView v, uint32_t col, const uint64_t* __restrict__ mask,
                                                               const uint64_t* __restrict__ bases, uint64_t ndeferred, uint32_t* __restrict__ list,
                                                               uint8_t* __restrict__ slots, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < v.nrows; i += stride) {
        const uint64_t word = mask[i >> 6];
        if (!((word >> lane) & 1)) continue;
        const uint64_t place = bases[i >> 6] + (uint64_t)__popcll(word & ((1ull << lane) - 1));
        const JsonlCell c = jsonl_cell(v, i, col);
        if (place >= ndeferred || !c.present) {
            bad |= kJlErrPlace;
            continue;
        }
        list[3 * place] = (uint32_t)i, list[3 * place + 1] = (uint32_t)(c.p - v.bytes), list[3 * place + 2] = c.n;
        const uint32_t take = c.n < kJlDeferSlot ? c.n : kJlDeferSlot;
        for (uint32_t k = 0; k < take; ++k) slots[place * kJlDeferSlot + k] = c.p[k];
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJlColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The deferred texts longer than a slot, one wave each: jobs[2 k] = where text k starts in the buffer | its length
// << 32, jobs[2 k + 1] = its place in `text` (the host checked both against the buffer and summed the lengths).
__global__ __launch_bounds__(256) void jsonl_defer_long_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ jobs, uint64_t njobs,
                                                               uint8_t* __restrict__ text) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < njobs; k += stride)  // uniform in the wave
        copy_span_wave(text + jobs[2 * k + 1], bytes + (uint32_t)jobs[2 * k], jobs[2 * k] >> 32, lane);
}

__global__ __launch_bounds__(256) void jsonl_defer_scatter_kernel(const uint32_t* __restrict__ list, const uint64_t* __restrict__ converted,
                                                                  uint64_t ndeferred, uint64_t nrows, uint64_t* __restrict__ values) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ndeferred; k += stride) {
        const uint32_t row = list[3 * k];
        if (row < nrows) values[row] = converted[k];
    }
}

// lens[i] (may be NULL) = the bytes of row i's string; validity (may be NULL); ctrl: the nulls, the unparsable
// cells and the bytes.
__global__ __launch_bounds__(256) void jsonl_str_len_kernel(const JsonlView v, uint32_t col, uint32_t* __restrict__ lens, uint8_t* __restrict__ validity,
                                                            unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = v.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: every lane reaches the ballots
    unsigned long long n_empty = 0, n_bad = 0, bytes = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        uint32_t kind = jsonl::kNull, len = 0;
        JsonlCell c{nullptr, 0, false};
        if (i < n) c = jsonl_cell(v, i, col);
        // a long cell between two quotes is looked through by the whole wave, 64 bytes a step: with no backslash, no
        // quote and no byte below 0x20 inside it is a string token of its own bytes, and no lane walks it
        const bool is_long = c.present && c.n >= kJlLongCell && c.p[0] == '"' && c.p[c.n - 1] == '"';
        bool plain = false;
        unsigned long long todo = __ballot(is_long);
        while (todo) {  // uniform in the wave
            const int from = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint8_t* p = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)c.p, from, 64);
            const uint32_t end = __shfl(c.n, from, 64) - 1;
            bool special = false;
            for (uint32_t at = 1 + lane; at < end; at += 64) {
                const uint32_t b = p[at];
                special |= b == '\\' || b == '"' || b < 0x20;
            }
            const bool any = __ballot(special) != 0;
            if ((int)lane == from) plain = !any;
        }
        if (plain) {
            kind = jsonl::kString, len = c.n - 2;
        } else if (c.present) {
            kind = jsonl::cell_kind(c.p, c.n, len);
            if (kind != jsonl::kString) len = kind == jsonl::kNull || kind == jsonl::kUnparsable ? 0 : c.n;
        }
        if (lens && i < n) lens[i] = len;
        const bool valid = kind != jsonl::kNull && kind != jsonl::kUnparsable;
        jsonl_store_word(validity, __ballot(valid), i - lane, n, lane);
        n_empty += __popcll(__ballot(i < n && kind == jsonl::kNull));
        n_bad += __popcll(__ballot(i < n && kind == jsonl::kUnparsable));
        unsigned long long sum = len;
#pragma unroll
        for (int off = 32; off; off >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, off, 64);
        bytes += sum;
    }
    if (lane == 0) {
        if (n_empty) atomicAdd(&ctrl[kJlColEmpty], n_empty);
        if (n_bad) atomicAdd(&ctrl[kJlColBad], n_bad);
        if (bytes) atomicAdd(&ctrl[kJlColBytes], bytes);
    }
}

// (lens are written and scanned into starts) offsets[0 .. n] and the bytes of every string.
__global__ __launch_bounds__(256) void jsonl_str_copy_kernel(const JsonlView v, uint32_t col, const uint32_t* __restrict__ lens,
                                                             const uint64_t* __restrict__ starts, uint64_t total, void* __restrict__ offsets,
                                                             uint32_t wide, uint8_t* __restrict__ values, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t n = v.nrows, stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform: the long cells are a whole wave's
    unsigned long long bad = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        uint64_t at = 0;
        uint32_t len = 0, raw = 0;
        const uint8_t* src = nullptr;  // the cell's text without the quotes of a string token
        bool escaped = false;
        JsonlCell c{nullptr, 0, false};
        if (i < n) {
            at = starts[i], len = lens[i];
            if (len) c = jsonl_cell(v, i, col);
            if (c.present) {
                const bool str = c.p[0] == '"' && c.n >= 2;
                src = str ? c.p + 1 : c.p, raw = str ? c.n - 2 : c.n;
                escaped = len != raw;
            }
            if (at + len > total || len > raw) bad |= kJlErrPlace, len = 0;  // never a store outside the total bytes
            if (wide) {
                ((uint64_t*)offsets)[i] = at;
                if (i + 1 == n) ((uint64_t*)offsets)[n] = total;
            } else {
                ((uint32_t*)offsets)[i] = (uint32_t)at;
                if (i + 1 == n) ((uint32_t*)offsets)[n] = (uint32_t)total;
            }
        }
        const bool is_long = len >= kJlLongCell && !escaped;
        if (len && !is_long) {
            if (escaped)
                (void)jsonl::unescape_copy(c.p, c.n, values + at, len);
            else
                copy_span_lane(values + at, src, len);
        }
        unsigned long long todo = __ballot(is_long);
        while (todo) {  // uniform in the wave
            const int from = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint8_t* p = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)src, from, 64);
            uint8_t* d = values + (uint64_t)__shfl((long long)at, from, 64);
            copy_span_wave(d, p, __shfl(len, from, 64), lane);
        }
    }
    if (bad) __hip_atomic_fetch_or(&ctrl[kJlColErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// bits[c] &= the class bits of every cell of column c among the first `rows` rows (bits start as all ones);
// some[c] |= 1 where a cell is not null.
__global__ __launch_bounds__(256) void jsonl_infer_kernel(const JsonlView v, uint64_t rows, uint32_t* __restrict__ bits, uint32_t* __restrict__ some) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (rows + stride - 1) / stride;  // uniform: every lane reaches the ballots
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t i = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        for (uint32_t c = 0; c < v.ncols; ++c) {
            uint32_t mine = csvnum::kAllOk;
            bool filled = false;
            if (i < rows) {
                const JsonlCell cell = jsonl_cell(v, i, c);
                if (cell.present) mine = jsonl::class_bits(cell.p, cell.n), filled = jsonl::cell_kind_shallow(cell.p, cell.n) != jsonl::kNull;
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
namespace jsonl = oxh::jsonl;
using oxh::JsonlView;

constexpr uint64_t kJsonlMagic = 0x4F58484A534C3031ull;  // "OXHJSL01"

struct JsonlHandle {
    uint64_t magic = kJsonlMagic;
    oxh_ctx* ctx = nullptr;
    int device = 0;
    const uint8_t* d_bytes = nullptr;
    uint8_t* owned = nullptr;   // the host form's device copy
    uint64_t nbytes = 0, infer_rows = 0;
    uint32_t* block = nullptr;  // ends | rec_end | row_rec | wf | canon
    uint32_t *ends = nullptr, *rec_end = nullptr, *row_rec = nullptr;
    uint64_t *wf = nullptr, *canon = nullptr;
    uint8_t* names_block = nullptr;  // the names' offsets (u32), then their bytes
    uint64_t nends = 0, nrec = 0, nrows = 0, ncols = 0;
    jsonl::Names names;
    ~JsonlHandle() {
        magic = 0;
        if (block) (void)hipFree(block);
        if (names_block) (void)hipFree(names_block);
        if (owned) (void)hipFree(owned);
    }
    JsonlView view() const {
        return JsonlView{d_bytes, ends, rec_end, row_rec, wf, canon, names_block ? names_block + (ncols + 1) * 4 : nullptr,
                         (const uint32_t*)names_block, nrows, (uint32_t)ncols};
    }
    uint64_t window() const { return std::min(infer_rows, nrows); }
};

unsigned cap_grid(uint64_t groups) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(groups, 1), 2048); }
unsigned row_grid(uint64_t n) { return cap_grid((n + 255) / 256); }

JsonlHandle* handle_of(void* p) {
    JsonlHandle* h = (JsonlHandle*)p;
    return h && h->magic == kJsonlMagic ? h : nullptr;
}

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

// The kept positions and the lines of h->d_bytes into h.
int index_run(JsonlHandle& h, hipStream_t st) {
    using namespace oxh;
    const uint64_t n = h.nbytes, mis = (uintptr_t)h.d_bytes & 15, lo = mis, hi = mis + n;
    const uint8_t* base = h.d_bytes - mis;
    const uint64_t tiles = csv::tiles_of(mis, n);
    if (csv::scan_tiles_of(tiles) != scan_tiles(tiles)) return fail(OXH_ERR_HIP, "jsonl: the scan's tile is not the lease's");
    const jsonl::IndexLease at(tiles);
    ScratchLease lease(st);  // ends (and waits for the stream) with this call
    void* lbase = nullptr;
    void* pinned = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess || lease.pinned(csv::kCtrlBytes, &pinned) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl: " + std::to_string(at.total) + " B of tile carries, counts and their scans");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    unsigned long long* h_ctrl = (unsigned long long*)pinned;
    uint32_t *d_esc = (uint32_t*)(b + at.esc), *d_esc_in = (uint32_t*)(b + at.esc_in), *d_flags = (uint32_t*)(b + at.flags);
    int32_t *d_d0 = (int32_t*)(b + at.d0), *d_d1 = (int32_t*)(b + at.d1);
    uint32_t* d_par_in = (uint32_t*)(b + at.par_in);
    int64_t* d_depth_in = (int64_t*)(b + at.depth_in);
    uint32_t *d_kept = (uint32_t*)(b + at.kept), *d_recs = (uint32_t*)(b + at.recs);
    uint64_t *d_kscan = (uint64_t*)(b + at.kept_scan), *d_rscan = (uint64_t*)(b + at.rec_scan);
    unsigned long long *d_ksums = (unsigned long long*)(b + at.kept_sums), *d_rsums = (unsigned long long*)(b + at.rec_sums);
    const unsigned grid = cap_grid(tiles);
    const uint64_t last = scan_tiles(tiles);
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kJlCtrlWords * 8, st));
        jsonl_esc_kernel<<<grid, 256, 0, st>>>(base, lo, hi, tiles, d_esc);
        HIP_TRY(hipGetLastError());
        jsonl_esc_carry_kernel<<<1, 256, 0, st>>>(d_esc, tiles, d_esc_in);
        HIP_TRY(hipGetLastError());
        jsonl_line_kernel<<<grid, 256, 0, st>>>(base, lo, hi, tiles, d_esc_in, d_flags, d_d0, d_d1);
        HIP_TRY(hipGetLastError());
        jsonl_line_carry_kernel<<<1, 256, 0, st>>>(d_flags, d_d0, d_d1, tiles, d_par_in, d_depth_in);
        HIP_TRY(hipGetLastError());
        jsonl_kept_kernel<false><<<grid, 256, 0, st>>>(base, lo, hi, tiles, d_esc_in, d_par_in, d_depth_in, d_kept, d_recs, nullptr, nullptr, nullptr,
                                                       nullptr, 0, 0, d_ctrl);
        HIP_TRY(hipGetLastError());
        int r = exclusive_scan_u32(d_kept, tiles, d_kscan, d_ksums, st);
        if (r) return r;
        if ((r = exclusive_scan_u32(d_recs, tiles, d_rscan, d_rsums, st))) return r;
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ksums + last, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ctrl + 1, d_rsums + last, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h.nends = h_ctrl[0], h.nrec = h_ctrl[1];
        if (h.nrec == 0 || h.nends < h.nrec || h.nends > n + 1)
            return fail(OXH_ERR_HIP, "jsonl: the kept counts are not those of a buffer (did it change during the call?)");
        // ends | rec_end | row_rec, then (8-byte aligned) a word per 64 rows of wf and of canon
        const uint64_t words32 = (h.nends + 2 * h.nrec + 1) & ~1ull, words64 = csv::blocks_of(h.nrec);
        const uint64_t bytes = words32 * 4 + 2 * words64 * 8;
        if (hipMalloc(&h.block, bytes) != hipSuccess) {
            (void)hipGetLastError();
            h.block = nullptr;
            return fail(OXH_ERR_NOMEM, "jsonl: " + std::to_string(bytes) + " B for the index");
        }
        poison_device(h.block, bytes, st);
        h.ends = h.block, h.rec_end = h.block + h.nends, h.row_rec = h.rec_end + h.nrec;
        h.wf = (uint64_t*)(h.block + words32), h.canon = h.wf + words64;
        jsonl_kept_kernel<true><<<grid, 256, 0, st>>>(base, lo, hi, tiles, d_esc_in, d_par_in, d_depth_in, nullptr, nullptr, d_kscan, d_rscan, h.ends,
                                                      h.rec_end, h.nends, h.nrec, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_ctrl[kJlCtrlErr]) return fail(OXH_ERR_HIP, "jsonl: a kept position's place is outside the index (did the buffer change during the call?)");
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// The row map and the well-formed bits; stats: the malformed records and the blank lines; first: the first
// well-formed row (nrows: none).
int rows_run(JsonlHandle& h, uint64_t& malformed, uint64_t& first, hipStream_t st) {
    using namespace oxh;
    const uint64_t blocks = csv::blocks_of(h.nrec);
    if (csv::scan_tiles_of(blocks) != scan_tiles(blocks)) return fail(OXH_ERR_HIP, "jsonl: the scan's tile is not the lease's");
    const csv::RowMapLease at(h.nrec);
    ScratchLease lease(st);
    void* lbase = nullptr;
    void* pinned = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess || lease.pinned(csv::kCtrlBytes, &pinned) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl: " + std::to_string(at.total) + " B of line masks and their scan");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    unsigned long long* h_ctrl = (unsigned long long*)pinned;
    uint64_t *d_mask = (uint64_t*)(b + at.mask), *d_bases = (uint64_t*)(b + at.bases);
    uint32_t* d_counts = (uint32_t*)(b + at.counts);
    unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kJlCtrlWords * 8, st));
        jsonl_keep_kernel<<<row_grid(h.nrec), 256, 0, st>>>(h.d_bytes, h.ends, h.rec_end, h.nrec, d_mask, d_counts);
        HIP_TRY(hipGetLastError());
        int r = exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st);
        if (r) return r;
        jsonl_rowmap_kernel<<<row_grid(h.nrec), 256, 0, st>>>(d_mask, d_bases, h.nrec, h.row_rec, d_ctrl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctrl + kJlCtrlWords, d_sums + scan_tiles(blocks), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h.nrows = h_ctrl[kJlCtrlWords];
        if (h.nrows > h.nrec) return fail(OXH_ERR_HIP, "jsonl: the row map is not that of the index");
        if (h.nrows) {
            jsonl_wellformed_kernel<<<row_grid(h.nrows), 256, 0, st>>>(h.d_bytes, h.ends, h.rec_end, h.row_rec, h.nrows, h.wf, d_ctrl);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, kJlCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_ctrl[kJlCtrlErr]) return fail(OXH_ERR_HIP, "jsonl: a record's place is outside the row map (did the buffer change during the call?)");
        malformed = h_ctrl[kJlCtrlMalformed];
        first = h_ctrl[kJlCtrlFirst] ? ~h_ctrl[kJlCtrlFirst] : h.nrows;
        if (malformed > h.nrows || first > h.nrows) return fail(OXH_ERR_HIP, "jsonl: the well-formed records are not those of the row map");
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// The names as they stand to the device, for the row kernels.
int names_upload(JsonlHandle& h, hipStream_t st) {
    if (h.names_block) (void)hipFree(h.names_block);
    h.names_block = nullptr;
    h.ncols = h.names.count();
    std::vector<uint32_t> offsets(h.ncols + 1);
    for (uint64_t c = 0; c <= h.ncols; ++c) offsets[c] = (uint32_t)h.names.offsets[c];
    const uint64_t bytes = offsets.size() * 4 + h.names.bytes.size();
    if (hipMalloc(&h.names_block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h.names_block = nullptr;
        return fail(OXH_ERR_NOMEM, "jsonl: " + std::to_string(bytes) + " B for the names on the device");
    }
    oxh::poison_device(h.names_block, bytes, st);
    HIP_TRY(hipMemcpyAsync(h.names_block, offsets.data(), offsets.size() * 4, hipMemcpyHostToDevice, st));
    if (!h.names.bytes.empty())
        HIP_TRY(hipMemcpyAsync(h.names_block + offsets.size() * 4, h.names.bytes.data(), h.names.bytes.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // the vectors end with this call
    return OXH_OK;
}

// The names and the canonical rows; counts3: the non-canonical rows, the ignored fields, the nested values.
int schema_run(JsonlHandle& h, uint64_t first, uint64_t* counts3, hipStream_t st) {
    using namespace oxh;
    const uint64_t window = h.window(), blocks = csv::blocks_of(window);
    if (csv::scan_tiles_of(window) != scan_tiles(window) || csv::scan_tiles_of(blocks) != scan_tiles(blocks))
        return fail(OXH_ERR_HIP, "jsonl: the scan's tile is not the lease's");
    const jsonl::SchemaLease at(window);
    ScratchLease lease(st);
    void* lbase = nullptr;
    void* pinned = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess || lease.pinned(csv::kCtrlBytes, &pinned) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl: " + std::to_string(at.total) + " B of listed rows, key counts and their scans");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    unsigned long long* h_ctrl = (unsigned long long*)pinned;
    uint64_t *d_mask = (uint64_t*)(b + at.mask), *d_bases = (uint64_t*)(b + at.bases);
    uint32_t *d_counts = (uint32_t*)(b + at.counts), *d_list = (uint32_t*)(b + at.list), *d_nkeys = (uint32_t*)(b + at.nkeys),
             *d_key_bytes = (uint32_t*)(b + at.key_bytes);
    uint64_t *d_nkeys_scan = (uint64_t*)(b + at.nkeys_scan), *d_bytes_scan = (uint64_t*)(b + at.bytes_scan);
    unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
    uint8_t* key_block = nullptr;
    // the keys of the nlist rows of d_list come down and join the names
    auto gather = [&](uint64_t nlist) -> int {
        const JsonlView v = h.view();
        jsonl_keys_len_kernel<<<row_grid(nlist), 256, 0, st>>>(v, d_list, nlist, d_nkeys, d_key_bytes);
        HIP_TRY(hipGetLastError());
        int r = exclusive_scan_u32(d_nkeys, nlist, d_nkeys_scan, d_sums, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(h_ctrl + kJlCtrlWords, d_sums + scan_tiles(nlist), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // d_sums is the next scan's too
        if ((r = exclusive_scan_u32(d_key_bytes, nlist, d_bytes_scan, d_sums, st))) return r;
        HIP_TRY(hipMemcpyAsync(h_ctrl + kJlCtrlWords + 1, d_sums + scan_tiles(nlist), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint64_t total_keys = h_ctrl[kJlCtrlWords], total_bytes = h_ctrl[kJlCtrlWords + 1];
        if (!total_keys) return OXH_OK;
        if (total_keys > h.nends || total_bytes > h.nbytes) return fail(OXH_ERR_HIP, "jsonl: the listed rows' keys are not those of the index");
        const uint64_t lens_bytes = csv::align256(total_keys * 4);
        if (hipMalloc(&key_block, lens_bytes + total_bytes) != hipSuccess) {
            (void)hipGetLastError();
            key_block = nullptr;
            return fail(OXH_ERR_NOMEM, "jsonl: " + std::to_string(lens_bytes + total_bytes) + " B for the listed rows' keys");
        }
        poison_device(key_block, lens_bytes + total_bytes, st);
        jsonl_keys_copy_kernel<<<row_grid(nlist), 256, 0, st>>>(v, d_list, nlist, d_nkeys_scan, d_bytes_scan, total_keys, total_bytes,
                                                               (uint32_t*)key_block, key_block + lens_bytes, d_ctrl);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> key_lens(total_keys);
        std::vector<uint8_t> text(total_bytes);
        HIP_TRY(hipMemcpyAsync(key_lens.data(), key_block, total_keys * 4, hipMemcpyDeviceToHost, st));
        if (total_bytes) HIP_TRY(hipMemcpyAsync(text.data(), key_block + lens_bytes, total_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        (void)hipFree(key_block);
        key_block = nullptr;
        if (h_ctrl[kJlCtrlErr]) return fail(OXH_ERR_HIP, "jsonl: a key's place is outside the listed keys (did the buffer change during the call?)");
        uint64_t sum = 0;
        for (uint32_t len : key_lens) sum += len;
        if (sum != total_bytes) return fail(OXH_ERR_HIP, "jsonl: the listed keys' lengths are not those measured");
        h.names.add_keys(key_lens.data(), total_keys, text.data());
        return OXH_OK;
    };
    auto canon = [&](bool list) -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kJlCtrlWords * 8, st));
        jsonl_canon_kernel<<<row_grid(h.nrows), 256, 0, st>>>(h.view(), h.canon, window, list ? d_mask : nullptr, list ? d_counts : nullptr, d_ctrl);
        HIP_TRY(hipGetLastError());
        return OXH_OK;
    };
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, kJlCtrlWords * 8, st));
        int r = names_upload(h, st);  // no names yet: the view is whole
        if (r) return r;
        if (first < window) {  // the first well-formed record's keys
            const uint32_t row = (uint32_t)first;
            HIP_TRY(hipMemcpyAsync(d_list, &row, 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
            if ((r = gather(1))) return r;
            if ((r = names_upload(h, st))) return r;
        }
        if ((r = canon(true))) return r;
        uint64_t nlist = 0;
        if (window) {
            if ((r = exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st))) return r;
            jsonl_rowmap_kernel<<<row_grid(window), 256, 0, st>>>(d_mask, d_bases, window, d_list, d_ctrl);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_ctrl + kJlCtrlWords, d_sums + scan_tiles(blocks), 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            nlist = h_ctrl[kJlCtrlWords];
            if (h_ctrl[kJlCtrlErr] || nlist > window) return fail(OXH_ERR_HIP, "jsonl: the listed rows are not those of the window");
        }
        if (nlist) {
            const uint64_t had = h.names.count();
            if ((r = gather(nlist))) return r;
            if (h.names.count() != had) {  // the names grew: the counts are against all of them
                if (h.names.count() > jsonl::kMaxNames) return OXH_OK;  // the caller refuses it
                if ((r = names_upload(h, st))) return r;
                if ((r = canon(false))) return r;
            }
        }
        HIP_TRY(hipMemcpyAsync(h_ctrl, d_ctrl, kJlCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        counts3[0] = h_ctrl[kJlCtrlNonCanon], counts3[1] = h_ctrl[kJlCtrlIgnored], counts3[2] = h_ctrl[kJlCtrlNested];
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    if (key_block) (void)hipFree(key_block);
    return rc;
}

// The index of h->d_bytes into h; stats8 is filled on success.
int open_run(JsonlHandle& h, uint64_t* stats8, hipStream_t st) {
    int rc = index_run(h, st);
    if (rc) return rc;
    uint64_t malformed = 0, first = 0, counts3[3] = {0, 0, 0};
    if ((rc = rows_run(h, malformed, first, st))) return rc;
    if (h.nrows && (rc = schema_run(h, first, counts3, st))) return rc;
    if (h.names.count() > jsonl::kMaxNames)
        return fail(OXH_ERR_INVALID, "jsonl open: " + std::to_string(h.names.count()) + " names (at most 65535)");
    h.ncols = h.names.count();
    stats8[0] = h.nrows, stats8[1] = h.nrows, stats8[2] = h.ncols, stats8[3] = malformed, stats8[4] = h.nrec - h.nrows;
    stats8[5] = counts3[0], stats8[6] = counts3[1], stats8[7] = counts3[2];
    STEP("jsonl open: %llu B, %llu lines, %llu rows x %llu columns", (unsigned long long)h.nbytes, (unsigned long long)h.nrec,
         (unsigned long long)h.nrows, (unsigned long long)h.ncols);
    return OXH_OK;
}

int open_enter(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint64_t infer_rows, uint32_t flags, void** out, uint64_t* stats8, bool& done) {
    done = false;
    const std::string what = jsonl::open_error(bytes, nbytes, infer_rows, flags, out, stats8);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "jsonl open: " + what);
    if (nbytes == 0) {  // a valid empty handle: no records, no columns
        JsonlHandle* h = new JsonlHandle;
        h->ctx = ctx, h->infer_rows = infer_rows;
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

// The measure: for every string column (and, with `all`, every other one) ctrl[k * kJlColWords ..] on the host.
int columns_measure(JsonlHandle& h, const Selection& s, bool all, std::vector<unsigned long long>& ctrl, hipStream_t st) {
    using namespace oxh;
    const JsonlView v = h.view();
    ctrl.assign((size_t)s.nsel * kJlColWords, 0);
    ScratchLease lease(st);
    void* lbase = nullptr;
    const uint64_t bytes = (uint64_t)s.nsel * kJlColWords * 8;
    if (lease.get(csv::align256(bytes), &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl columns: " + std::to_string(bytes) + " B of control words");
    }
    unsigned long long* d_ctrl = (unsigned long long*)lbase;
    const unsigned grid = row_grid(h.nrows);
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, bytes, st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            unsigned long long* c = d_ctrl + (size_t)k * kJlColWords;
            const uint32_t col = s.col_idx[k];
            if (csv::is_string(s.types[k]))
                jsonl_str_len_kernel<<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, c);
            else if (!all)
                continue;
            else if (s.types[k] == OXH_CSV_INT64)
                jsonl_fixed_kernel<OXH_CSV_INT64><<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, nullptr, nullptr, nullptr, c);
            else if (s.types[k] == OXH_CSV_FLOAT64)
                jsonl_fixed_kernel<OXH_CSV_FLOAT64><<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, nullptr, nullptr, nullptr, c);
            else
                jsonl_fixed_kernel<OXH_CSV_BOOL><<<grid, 256, 0, st>>>(v, col, nullptr, nullptr, nullptr, nullptr, nullptr, c);
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
int convert_deferred(JsonlHandle& h, uint32_t col, uint64_t ndeferred, const uint64_t* d_mask, const uint32_t* d_counts, uint64_t* d_bases,
                     unsigned long long* d_sums, unsigned long long* d_ctrl, uint64_t* d_values, hipStream_t st) {
    using namespace oxh;
    const JsonlView v = h.view();
    const uint64_t blocks = csv::blocks_of(h.nrows);
    const uint64_t list_bytes = csv::align256(ndeferred * 12), slot_bytes = csv::align256(ndeferred * kJlDeferSlot), value_bytes = ndeferred * 8;
    uint8_t* block = nullptr;
    if (hipMalloc(&block, list_bytes + slot_bytes + value_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl columns: " + std::to_string(list_bytes + slot_bytes + value_bytes) + " B for the deferred cells");
    }
    poison_device(block, list_bytes + slot_bytes + value_bytes, st);
    uint32_t* d_list = (uint32_t*)block;
    uint8_t* d_slots = block + list_bytes;
    uint64_t* d_converted = (uint64_t*)(block + list_bytes + slot_bytes);
    std::vector<uint32_t> list(ndeferred * 3);
    std::vector<uint8_t> slots(ndeferred * kJlDeferSlot);
    std::vector<uint64_t> converted(ndeferred);
    uint8_t* long_block = nullptr;  // the jobs and the bytes of the texts longer than a slot, where there are any
    int rc = [&]() -> int {
        int r = exclusive_scan_u32(d_counts, blocks, d_bases, d_sums, st);
        if (r) return r;
        jsonl_defer_emit_kernel<<<row_grid(h.nrows), 256, 0, st>>>(v, col, d_mask, d_bases, ndeferred, d_list, d_slots, d_ctrl);
        HIP_TRY(hipGetLastError());
        unsigned long long err = 0;
        HIP_TRY(hipMemcpyAsync(list.data(), d_list, list.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(slots.data(), d_slots, slots.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&err, d_ctrl + kJlColErr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (err) return fail(OXH_ERR_HIP, "jsonl columns: a deferred cell's place is outside the list (did the buffer change during the call?)");
        std::vector<uint64_t> jobs;  // per long text: where it starts | its length << 32, then its place in `text`
        uint64_t long_bytes = 0;
        for (uint64_t k = 0; k < ndeferred; ++k) {
            const uint32_t start = list[3 * k + 1], len = list[3 * k + 2];
            if ((uint64_t)start + len > h.nbytes) return fail(OXH_ERR_HIP, "jsonl columns: a deferred cell is not inside the buffer");
            if (len <= kJlDeferSlot) continue;
            jobs.push_back(start | (uint64_t)len << 32), jobs.push_back(long_bytes);
            long_bytes += len;
        }
        std::vector<char> text(long_bytes);
        if (!jobs.empty()) {
            const uint64_t job_bytes = jobs.size() * 8;
            if (hipMalloc(&long_block, job_bytes + long_bytes) != hipSuccess) {
                (void)hipGetLastError();
                long_block = nullptr;
                return fail(OXH_ERR_NOMEM, "jsonl columns: " + std::to_string(job_bytes + long_bytes) + " B for the long deferred texts");
            }
            poison_device(long_block, job_bytes + long_bytes, st);
            HIP_TRY(hipMemcpyAsync(long_block, jobs.data(), job_bytes, hipMemcpyHostToDevice, st));
            jsonl_defer_long_kernel<<<cap_grid((jobs.size() / 2 + 3) / 4), 256, 0, st>>>(h.d_bytes, (const uint64_t*)long_block, jobs.size() / 2,
                                                                                          long_block + job_bytes);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(text.data(), long_block + job_bytes, long_bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        uint64_t long_at = 0;
        for (uint64_t k = 0; k < ndeferred; ++k) {
            const uint32_t len = list[3 * k + 2];
            const char* p = (const char*)slots.data() + k * kJlDeferSlot;
            if (len > kJlDeferSlot) p = text.data() + long_at, long_at += len;
            const double x = csv::convert_deferred(p, len);
            memcpy(&converted[k], &x, 8);
        }
        HIP_TRY(hipMemcpyAsync(d_converted, converted.data(), value_bytes, hipMemcpyHostToDevice, st));
        jsonl_defer_scatter_kernel<<<row_grid(ndeferred), 256, 0, st>>>(d_list, d_converted, ndeferred, h.nrows, d_values);
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
int columns_write(JsonlHandle& h, const Selection& s, const std::vector<uint64_t>& string_bytes, void* const* d_values, void* const* d_offsets,
                  uint8_t* const* d_validity, std::vector<unsigned long long>& ctrl, hipStream_t st) {
    using namespace oxh;
    const JsonlView v = h.view();
    const uint64_t n = h.nrows;
    if (csv::scan_tiles_of(n) != scan_tiles(n)) return fail(OXH_ERR_HIP, "jsonl: the scan's tile is not the lease's");
    const csv::ColumnsLease at(n, s.nsel, s.types, true);
    ctrl.assign((size_t)s.nsel * kJlColWords, 0);
    ScratchLease lease(st);
    void* lbase = nullptr;
    if (lease.get(at.total, &lbase) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl columns: " + std::to_string(at.total) + " B of lengths, their scan and the deferred masks");
    }
    uint8_t* b = (uint8_t*)lbase;
    unsigned long long* d_ctrl = (unsigned long long*)(b + at.ctrl);
    uint32_t* d_lens = (uint32_t*)(b + at.lens);
    uint64_t* d_len_scan = (uint64_t*)(b + at.len_scan);
    unsigned long long* d_sums = (unsigned long long*)(b + at.sums);
    const uint64_t ctrl_bytes = (uint64_t)s.nsel * kJlColWords * 8;
    const unsigned grid = row_grid(n);
    int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_ctrl, 0, ctrl_bytes, st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            unsigned long long* c = d_ctrl + (size_t)k * kJlColWords;
            const uint32_t col = s.col_idx[k], type = s.types[k];
            if (csv::is_string(type)) {
                jsonl_str_len_kernel<<<grid, 256, 0, st>>>(v, col, d_lens, d_validity[k], c);
                HIP_TRY(hipGetLastError());
                int r = exclusive_scan_u32(d_lens, n, d_len_scan, d_sums, st);
                if (r) return r;
                jsonl_str_copy_kernel<<<grid, 256, 0, st>>>(v, col, d_lens, d_len_scan, string_bytes[k], d_offsets[k], type == OXH_CSV_STRING64,
                                                            (uint8_t*)d_values[k], c);
            } else if (type == OXH_CSV_INT64) {
                jsonl_fixed_kernel<OXH_CSV_INT64><<<grid, 256, 0, st>>>(v, col, (uint64_t*)d_values[k], nullptr, d_validity[k], nullptr, nullptr, c);
            } else if (type == OXH_CSV_FLOAT64) {
                jsonl_fixed_kernel<OXH_CSV_FLOAT64><<<grid, 256, 0, st>>>(v, col, (uint64_t*)d_values[k], nullptr, d_validity[k],
                                                                          (uint64_t*)(b + at.defer_mask[k]), (uint32_t*)(b + at.defer_counts[k]), c);
            } else {
                jsonl_fixed_kernel<OXH_CSV_BOOL><<<grid, 256, 0, st>>>(v, col, nullptr, (uint8_t*)d_values[k], d_validity[k], nullptr, nullptr, c);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(ctrl.data(), d_ctrl, ctrl_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < s.nsel; ++k) {
            const unsigned long long* c = ctrl.data() + (size_t)k * kJlColWords;
            if (c[kJlColErr]) return fail(OXH_ERR_HIP, "jsonl columns: a string's place is outside its column's bytes (did the buffer change during the call?)");
            if (csv::is_string(s.types[k]) && c[kJlColBytes] != string_bytes[k]) return fail(OXH_ERR_HIP, "jsonl columns: a column's bytes are not those measured");
            if (s.types[k] == OXH_CSV_FLOAT64 && c[kJlColDeferred]) {
                int r = convert_deferred(h, s.col_idx[k], c[kJlColDeferred], (const uint64_t*)(b + at.defer_mask[k]), (const uint32_t*)(b + at.defer_counts[k]),
                                         (uint64_t*)(b + at.defer_bases), d_sums, d_ctrl + (size_t)k * kJlColWords, (uint64_t*)d_values[k], st);
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
        const unsigned long long* c = ctrl.data() + (size_t)k * kJlColWords;
        value_bytes[k] = csv::is_string(s.types[k]) ? c[kJlColBytes] : csv::fixed_value_bytes(s.types[k], nrows);
        stats4[4 * k] = c[kJlColEmpty], stats4[4 * k + 1] = c[kJlColBad], stats4[4 * k + 2] = c[kJlColDeferred], stats4[4 * k + 3] = value_bytes[k];
    }
}

// What both forms of oxh_jsonl_columns_* do first. `done`: nothing left to do.
int columns_enter(void* handle, const csv::ColumnsArgs& a, JsonlHandle*& h, bool& done) {
    done = false;
    h = handle_of(handle);
    if (!h) return fail(OXH_ERR_INVALID, "jsonl columns: the handle is NULL or not a JSON Lines handle");
    csv::ColumnsArgs full = a;
    full.nrows = h->nrows, full.ncols = h->ncols;
    const std::string what = csv::columns_error(full);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "jsonl columns: " + what);
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
int columns_run(JsonlHandle& h, const csv::ColumnsArgs& a, void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity,
                const uint64_t* capacity, hipStream_t st, const std::vector<uint64_t>* measured = nullptr) {
    const Selection s{a.nsel, a.col_idx, a.types};
    const bool write = d_values != nullptr;
    bool strings = false;
    for (uint32_t k = 0; k < a.nsel; ++k) strings |= csv::is_string(a.types[k]);
    std::vector<unsigned long long> ctrl((size_t)a.nsel * oxh::kJlColWords, 0);
    std::vector<uint64_t> string_bytes(a.nsel, 0);
    if (measured) {
        string_bytes = *measured;
    } else if (strings || !write) {
        int rc = columns_measure(h, s, !write, ctrl, st);
        if (rc) return rc;
        for (uint32_t k = 0; k < a.nsel; ++k) {
            if (!csv::is_string(a.types[k])) continue;
            string_bytes[k] = ctrl[(size_t)k * oxh::kJlColWords + oxh::kJlColBytes];
            const std::string what = csv::string_bytes_error(a.types[k], string_bytes[k], write, write ? capacity[k] : 0);
            if (!what.empty()) return fail(OXH_ERR_INVALID, "jsonl columns: selection " + std::to_string(k) + ": " + what);
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

int oxh_jsonl_open_device(oxh_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, uint64_t infer_rows, uint32_t flags, void** out, uint64_t* stats8,
                          void* stream) {
    bool done = false;
    int rc = open_enter(ctx, d_bytes, nbytes, infer_rows, flags, out, stats8, done);
    if (rc || done) return rc;
    std::unique_ptr<JsonlHandle> h(new JsonlHandle);
    h->ctx = ctx, h->device = ctx->device, h->d_bytes = d_bytes, h->nbytes = nbytes, h->infer_rows = infer_rows;
    uint64_t stats[8] = {};
    rc = open_run(*h, stats, (hipStream_t)stream);
    if (rc) return rc;
    memcpy(stats8, stats, sizeof stats);
    *out = h.release();
    return OXH_OK;
}

int oxh_jsonl_open_host(oxh_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint64_t infer_rows, uint32_t flags, void** out, uint64_t* stats8) {
    bool done = false;
    int rc = open_enter(ctx, bytes, nbytes, infer_rows, flags, out, stats8, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    std::unique_ptr<JsonlHandle> h(new JsonlHandle);
    h->ctx = ctx, h->device = ctx->device, h->nbytes = nbytes, h->infer_rows = infer_rows;
    // the copy keeps the caller's phase within 16 bytes: the aligned loads fall where they would on the caller's buffer
    const uint64_t phase = (uintptr_t)bytes & 15;
    if (hipMalloc(&h->owned, nbytes + 32) != hipSuccess) {
        (void)hipGetLastError();
        h->owned = nullptr;
        return fail(OXH_ERR_NOMEM, "jsonl open: " + std::to_string(nbytes) + " B for the file on the device");
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

int oxh_jsonl_close(void* jsonl_handle) {
    if (!jsonl_handle) return OXH_OK;
    JsonlHandle* h = handle_of(jsonl_handle);
    if (!h) return fail(OXH_ERR_INVALID, "jsonl close: not a JSON Lines handle");
    if (h->block || h->owned || h->names_block) (void)hipSetDevice(h->device);
    delete h;
    return OXH_OK;
}

int oxh_jsonl_names(void* jsonl_handle, uint8_t* names, uint64_t capacity, uint64_t* name_offsets, uint64_t* names_bytes) {
    JsonlHandle* h = handle_of(jsonl_handle);
    if (!h) return fail(OXH_ERR_INVALID, "jsonl names: the handle is NULL or not a JSON Lines handle");
    if (!name_offsets || !names_bytes) return fail(OXH_ERR_INVALID, "jsonl names: name_offsets or names_bytes is NULL");
    *names_bytes = h->names.bytes.size();
    if (!names || capacity < h->names.bytes.size()) return OXH_OK;
    if (!h->names.bytes.empty()) memcpy(names, h->names.bytes.data(), h->names.bytes.size());
    for (uint64_t c = 0; c <= h->ncols; ++c) name_offsets[c] = h->names.offsets[c];
    return OXH_OK;
}

int oxh_jsonl_infer(void* jsonl_handle, uint32_t* types) {
    using namespace oxh;
    JsonlHandle* h = handle_of(jsonl_handle);
    if (!h) return fail(OXH_ERR_INVALID, "jsonl infer: the handle is NULL or not a JSON Lines handle");
    if (h->ncols && !types) return fail(OXH_ERR_INVALID, "jsonl infer: types is NULL");
    const uint64_t rows = h->window(), ncols = h->ncols;
    if (!rows || !ncols) {
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
            return fail(OXH_ERR_NOMEM, "jsonl infer: " + std::to_string(ncols * 8) + " B of class bits");
        }
        uint32_t* d_bits = (uint32_t*)lbase;
        rc = [&]() -> int {
            HIP_TRY(hipMemsetAsync(d_bits, 0xFF, ncols * 4, st));
            HIP_TRY(hipMemsetAsync(d_bits + ncols, 0, ncols * 4, st));
            jsonl_infer_kernel<<<row_grid(rows), 256, 0, st>>>(h->view(), rows, d_bits, d_bits + ncols);
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
    for (uint64_t c = 0; c < ncols; ++c) types[c] = jsonl::type_of_bits(words[c] & csvnum::kAllOk, words[ncols + c] == 0);
    return OXH_OK;
}

int oxh_jsonl_columns_device(void* jsonl_handle, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                             void* const* d_values, void* const* d_offsets, uint8_t* const* d_validity, uint64_t* value_bytes, uint64_t* stats4,
                             void* stream) {
    const csv::ColumnsArgs a{0, 0, nsel, col_idx, types, value_capacity, d_values, d_offsets, d_validity, value_bytes, stats4};
    JsonlHandle* h = nullptr;
    bool done = false;
    int rc = columns_enter(jsonl_handle, a, h, done);
    if (rc || done) return rc;
    return columns_run(*h, a, d_values, d_offsets, d_validity, value_capacity, (hipStream_t)stream);
}

int oxh_jsonl_columns_host(void* jsonl_handle, uint32_t nsel, const uint32_t* col_idx, const uint32_t* types, const uint64_t* value_capacity,
                           void* const* values, void* const* offsets, uint8_t* const* validity, uint64_t* value_bytes, uint64_t* stats4) {
    const csv::ColumnsArgs a{0, 0, nsel, col_idx, types, value_capacity, values, offsets, validity, value_bytes, stats4};
    JsonlHandle* h = nullptr;
    bool done = false;
    int rc = columns_enter(jsonl_handle, a, h, done);
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
            if (csv::is_string(types[k])) bytes[k] = ctrl[(size_t)k * oxh::kJlColWords + oxh::kJlColBytes];
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
            if (!what.empty()) return fail(OXH_ERR_INVALID, "jsonl columns: selection " + std::to_string(k) + ": " + what);
            offset_bytes[k] = (n + 1) * (types[k] == OXH_CSV_STRING64 ? 8 : 4);
        }
        at_values[k] = carve(bytes[k]), at_offsets[k] = carve(offset_bytes[k]), at_validity[k] = carve(bitmap);
    }
    uint8_t* d_block = nullptr;
    if (hipMalloc(&d_block, total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "jsonl columns: " + std::to_string(total) + " B for the columns on the device");
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
