// oxen_amd/csrc/embedding.hip -- the embedding query of a data frame (oxh_embedding_*): `oxen df
// --find-embedding-where "id = 42" --sort-by-similarity-to embedding` and the server's nearest neighbours
// (repositories/workspaces/data_frames/embeddings.rs: :569-641 get_avg_embedding, :331-358
// build_similarity_query_sql, :413-567 query / nearest_neighbors) over a column of float32 vectors on the device.
// The semantics are stated in include/oxen_hash.h (DESIGN.md §4 "Embedding similarity"); the argument checks,
// the order key, the mean's partition and the host forms' staging are embedding_host.hpp's, the code
// tests/native/embedding_host_test.cpp runs on the host.
//
//   mean        emb_mean_partial_kernel: the lanes of a workgroup across dim (coalesced), the workgroups across
//               chunks of idx; every workgroup leaves one row of partial sums. emb_mean_finish_kernel, a later
//               launch, adds those rows in their order and divides by the rows used. No floating-point atomic:
//               the result depends on nidx and dim alone.
//   similarity  emb_similarity_kernel<LPR>: LPR lanes per row -- 4 for dim <= kEmbQuadDimMax, 16 up to
//               kEmbSubwaveDimMax, else the whole wave. The query sits in LDS and its norm is summed once per
//               workgroup. A wave takes a task of neighbouring rows (64, or 8 with a wave per row), four rows per
//               lane group in flight: the 4-byte elements up to the first 16-byte boundary of the row, 16-byte
//               loads from there, the 4-byte rest. The three sums are reduced by shuffles inside the lane group;
//               lane L of the wave collects row L of the task and stores sim and the order key (coalesced), and
//               the ballot of the valid rows gives the validity bytes: a byte has one writer.
//   order       the stable ascending sort of the order keys is oxh_sort_rows_device over that one column, called
//               after the similarity's lease has ended (leases do not nest).
//   take        emb_take_rows_kernel (validity bytes and counts, a lane per output row) and
//               emb_take_values_kernel (a lane per output float).
// A row is never read through a bad pair of offsets, through a span of another length than dim, or through an
// index that is not a row: such a row counts, the call finishes and returns OXH_ERR_INVALID.
#include "capi_internal.hpp"
#include "columns.hpp"
#include "embedding_host.hpp"

using namespace oxh::capi;

namespace oxh {

namespace emb = oxh::embedding;

// lanes per row by dim: a quarter-wave's 16 float4 loads cover 64 floats, a whole wave's 256. Below
// kEmbQuadDimMax + 1 floats a row is at most one 16-byte load and its edges: 4 lanes hold it.
constexpr uint32_t kEmbQuadDimMax = 16, kEmbSubwaveDimMax = 256;
constexpr uint32_t kEmbQueryLds = 12288;      // floats of a query kept in LDS (48 KiB); a longer one is read through the caches
constexpr int kEmbRowsInFlight = 4;           // rows a lane group loads side by side
constexpr uint32_t kEmbGridCap = 2048;

// ctrl words of one call
constexpr int kEmbCtrlErr = 0, kEmbCtrlUsed = 1, kEmbCtrlNull = 2, kEmbCtrlWrong = 3, kEmbCtrlFirstWrong = 4, kEmbCtrlWords = 5;
constexpr unsigned long long kEmbErrOffsets = 1, kEmbErrIndex = 2;
constexpr uint32_t kRowOk = 0, kRowNull = 1, kRowWrong = 2, kRowBadOffsets = 3, kRowBadIndex = 4, kRowAbsent = 5;

// The column as the kernels get it. Rows below row0 and elements below elem0 are not there (a host form stages
// only the span its rows name): offsets and validity are addressed by r - row0, values by element - elem0.
struct EmbCol {
    const float* values;
    const uint8_t* offsets;
    const uint8_t* validity;
    uint64_t nbit;
    uint64_t row0, elem0;
    uint64_t nrows;
    uint32_t dim;
    uint32_t layout;
};

// Row r (row0 <= r < nrows): kRowOk with `start` = where its dim floats begin in c.values, or why it is not read.
__device__ __forceinline__ uint32_t emb_row(const EmbCol& c, uint64_t r, uint64_t& start) {
    const uint64_t k = r - c.row0;
    if (c.validity && !row_bit(c.validity, c.nbit + k)) return kRowNull;
    if (c.layout == OXH_EMB_FIXED) {
        start = r * c.dim - c.elem0;
        return kRowOk;
    }
    int64_t s, e;
    if (c.layout == OXH_EMB_LIST32) {
        s = (int32_t)ld32u(c.offsets + 4 * k);
        e = (int32_t)ld32u(c.offsets + 4 * k + 4);
    } else {
        s = (int64_t)ld64u(c.offsets + 8 * k);
        e = (int64_t)ld64u(c.offsets + 8 * k + 8);
    }
    if (s < 0 || e < s || (uint64_t)s < c.elem0) return kRowBadOffsets;  // never a read through such a pair
    if ((uint64_t)(e - s) != c.dim) return kRowWrong;                   // nor through a span of another length
    start = (uint64_t)s - c.elem0;
    return kRowOk;
}

// What the rows of a wave were, added to the wave's counts (the same in every lane).
struct EmbCounts {
    unsigned long long used = 0, nulls = 0, wrong = 0, first_wrong = ~0ull, bad = 0;
    __device__ __forceinline__ void add(uint32_t state, bool live, uint64_t my_row) {
        used += __popcll(__ballot(live && state == kRowOk));
        nulls += __popcll(__ballot(live && state == kRowNull));
        const unsigned long long w = __ballot(live && state == kRowWrong);
        wrong += __popcll(w);
        // the smallest row among the wrong ones of this wave step
        unsigned long long mine = live && state == kRowWrong ? my_row : ~0ull;
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)mine, m, 64);
            mine = other < mine ? other : mine;
        }
        if (w && mine < first_wrong) first_wrong = mine;
        if (__ballot(live && state == kRowBadOffsets)) bad |= kEmbErrOffsets;
        if (__ballot(live && state == kRowBadIndex)) bad |= kEmbErrIndex;
    }
    __device__ __forceinline__ void flush(unsigned long long* ctrl, unsigned lane) {
        if (lane != 0) return;
        if (used) atomicAdd(&ctrl[kEmbCtrlUsed], used);
        if (nulls) atomicAdd(&ctrl[kEmbCtrlNull], nulls);
        if (wrong) {
            atomicAdd(&ctrl[kEmbCtrlWrong], wrong);
            atomicMin(&ctrl[kEmbCtrlFirstWrong], first_wrong);
        }
        if (bad) __hip_atomic_fetch_or(&ctrl[kEmbCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---------------------------------------------------------------- mean
// partial[g * dim + d] = the sum over workgroup g's chunks (g, g + G, ..: embedding_host.hpp) of element d of the
// used rows. `lanes` (a power of two, 256 when dim is above it) lanes stand across dim, the 256 / lanes groups of
// them take every (256 / lanes)-th idx entry of a chunk and are added in their order in LDS.
__global__ __launch_bounds__(256) void emb_mean_partial_kernel(const EmbCol c, const uint32_t* __restrict__ idx, uint64_t nidx, uint32_t lanes,
                                                               float* __restrict__ partial, unsigned long long* __restrict__ ctrl) {
    __shared__ float red[256];
    const uint32_t col = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, nsub = 256 / lanes;
    const uint64_t chunks = (nidx + emb::kMeanChunk - 1) / emb::kMeanChunk;
    unsigned long long used = 0, nulls = 0, wrong = 0, first_wrong = ~0ull, bad = 0;  // of the lanes with col == 0, first tile
    for (uint32_t d0 = 0; d0 < c.dim; d0 += lanes) {
        const uint32_t d = d0 + col;
        float acc = 0.0f;
        for (uint64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
            const uint64_t lo = ch * emb::kMeanChunk, hi = lo + emb::kMeanChunk < nidx ? lo + emb::kMeanChunk : nidx;
#pragma unroll 4
            for (uint64_t i = lo + sub; i < hi; i += nsub) {
                const uint64_t r = idx[i];
                uint64_t start = 0;
                const uint32_t state = r >= c.nrows || r < c.row0 ? kRowBadIndex : emb_row(c, r, start);  // an index that is no row: nothing is read
                if (state == kRowOk && d < c.dim) acc += c.values[start + d];
                if (d0 == 0 && col == 0) {
                    used += state == kRowOk, nulls += state == kRowNull;
                    if (state == kRowWrong) {
                        ++wrong;
                        first_wrong = r < first_wrong ? r : first_wrong;
                    }
                    if (state == kRowBadOffsets) bad |= kEmbErrOffsets;
                    if (state == kRowBadIndex) bad |= kEmbErrIndex;
                }
            }
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (sub == 0 && d < c.dim) {
            float s = red[col];
            for (uint32_t k = 1; k < nsub; ++k) s += red[col + k * lanes];
            partial[(uint64_t)blockIdx.x * c.dim + d] = s;
        }
        __syncthreads();
    }
    if (col == 0) {
        if (used) atomicAdd(&ctrl[kEmbCtrlUsed], used);
        if (nulls) atomicAdd(&ctrl[kEmbCtrlNull], nulls);
        if (wrong) {
            atomicAdd(&ctrl[kEmbCtrlWrong], wrong);
            atomicMin(&ctrl[kEmbCtrlFirstWrong], first_wrong);
        }
        if (bad) __hip_atomic_fetch_or(&ctrl[kEmbCtrlErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// (the partial sums are written, the counts have landed) out[d] = (partial[0][d] + partial[1][d] + ..) / used, the
// rows of partial in their order; nothing is stored when no row was used.
__global__ __launch_bounds__(256) void emb_mean_finish_kernel(const float* __restrict__ partial, uint32_t groups, uint32_t dim,
                                                              const unsigned long long* __restrict__ ctrl, float* __restrict__ out) {
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long used = ctrl[kEmbCtrlUsed];
    if (d >= dim || used == 0) return;
    float s = 0.0f;
#pragma unroll 8
    for (uint32_t g = 0; g < groups; ++g) s += partial[(uint64_t)g * dim + d];
    out[d] = s / (float)used;
}

// ---------------------------------------------------------------- similarity
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// dot[u] += sum x q and nx[u] += sum x x over the elements of U rows that lane j of an LPR-lane group takes:
// of row u (at p[u], read only when live[u]) the elements in front of the first 16-byte boundary (at most 3, one
// lane each), then 16-byte pieces j, j + LPR, .., then the rest (at most 3). The U rows' loads of one step are
// issued together.
template <int LPR, int U>
__device__ __forceinline__ void rows_sums(const float* (&p)[U], const bool (&live)[U], uint32_t dim, unsigned j, const float* q,
                                          float (&dot)[U], float (&nx)[U]) {
    uint32_t head[U], nbody[U], most = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t to_boundary = (uint32_t)((16 - ((uintptr_t)p[u] & 15)) & 15) >> 2;
        head[u] = !live[u] ? 0 : to_boundary < dim ? to_boundary : dim;
        nbody[u] = live[u] ? (dim - head[u]) >> 2 : 0;
        most = nbody[u] > most ? nbody[u] : most;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (live[u] && j < head[u]) {
            const float x = p[u][j];
            dot[u] += x * q[j], nx[u] += x * x;
        }
        const uint32_t rest = head[u] + 4 * nbody[u] + j;  // j < 3 names every element of the rest
        if (live[u] && j < 3 && rest < dim) {
            const float x = p[u][rest];
            dot[u] += x * q[rest], nx[u] += x * x;
        }
    }
    for (uint32_t k = j; k < most; k += LPR) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            v[u] = k < nbody[u] ? *reinterpret_cast<const float4*>(p[u] + head[u] + 4 * k) : float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k >= nbody[u]) continue;
            const float* qk = q + head[u] + 4 * k;
            dot[u] += v[u].x * qk[0] + v[u].y * qk[1] + v[u].z * qk[2] + v[u].w * qk[3];
            nx[u] += v[u].x * v[u].x + v[u].y * v[u].y + v[u].z * v[u].z + v[u].w * v[u].w;
        }
    }
}

// sim[r], order_key[r] (may be NULL) and the validity bytes (may be NULL) of every row. A task is TASK neighbouring
// rows of one wave, a multiple of 8: the task's validity bytes are its own.
template <int LPR, bool QLDS>
__global__ __launch_bounds__(256) void emb_similarity_kernel(const EmbCol c, const float* __restrict__ query, float* __restrict__ sim,
                                                             uint8_t* __restrict__ sim_validity, uint32_t* __restrict__ order_key,
                                                             unsigned long long* __restrict__ ctrl) {
    constexpr int TASK = LPR == 64 ? 8 : 64;   // rows of a task: lane L < TASK collects row L
    constexpr int RPS = 64 / LPR;              // rows of one step: one per lane group
    constexpr int STEPS = TASK / RPS, U = kEmbRowsInFlight;
    static_assert(STEPS % U == 0 && TASK % 8 == 0, "a task is whole rounds of U steps and whole validity bytes");
    extern __shared__ float sq[];
    __shared__ float part[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {   // the query into LDS, and its norm once per workgroup
        float acc = 0.0f;
        for (uint32_t i = threadIdx.x; i < c.dim; i += 256) {
            const float v = query[i];
            if (QLDS) sq[i] = v;
            acc += v * v;
        }
        acc = group_sum<64>(acc);
        if (lane == 0) part[wave] = acc;
        __syncthreads();
    }
    const float nq = (part[0] + part[1]) + (part[2] + part[3]);
    const float* q = QLDS ? sq : query;
    const unsigned j = lane % LPR, g = lane / LPR;
    const uint64_t ntasks = (c.nrows + TASK - 1) / TASK;
    EmbCounts counts;
    for (uint64_t task = (uint64_t)blockIdx.x * 4 + wave; task < ntasks; task += (uint64_t)gridDim.x * 4) {
        const uint64_t base = task * TASK, my_row = base + lane;
        const bool mine = lane < TASK && my_row < c.nrows;
        uint64_t my_start = 0;
        const uint32_t my_state = mine ? emb_row(c, my_row, my_start) : kRowAbsent;
        float my_sim = 0.0f;
        for (int s0 = 0; s0 < STEPS; s0 += U) {
            const float* p[U];
            bool live[U];
            float dot[U], nx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = (s0 + u) * RPS + (int)g;  // the lane that holds this group's row of step s0 + u
                const uint32_t state = (uint32_t)__shfl((int)my_state, src, 64);
                const uint64_t start = (uint64_t)__shfl((long long)my_start, src, 64);
                live[u] = state == kRowOk;
                p[u] = c.values + (live[u] ? start : 0);
                dot[u] = nx[u] = 0.0f;
            }
            rows_sums<LPR, U>(p, live, c.dim, j, q, dot, nx);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float d = group_sum<LPR>(dot[u]), n = group_sum<LPR>(nx[u]);
                float s = d / sqrtf(n * nq);
                if (s > 1.0f) s = 1.0f;    // a NaN passes both
                if (s < -1.0f) s = -1.0f;
                const float v = __shfl(s, (int)(lane % RPS) * LPR, 64);
                if ((int)(lane / RPS) == s0 + u) my_sim = v;
            }
        }
        const bool ok = my_state == kRowOk;
        if (mine) {
            const float s = ok ? my_sim : 0.0f;
            sim[my_row] = s;
            if (order_key) order_key[my_row] = ok ? emb::order_key(__float_as_uint(s)) : emb::kNullKey;
        }
        const unsigned long long valid = __ballot(ok);
        if (sim_validity && lane < TASK / 8 && base + 8 * lane < c.nrows) sim_validity[(base >> 3) + lane] = (uint8_t)(valid >> (8 * lane));
        counts.add(my_state, mine, my_row);
    }
    counts.flush(ctrl, lane);
}

// ---------------------------------------------------------------- take
// The validity bytes of the page and what its rows were: a lane per output row, a wave on 64 neighbouring rows.
__global__ __launch_bounds__(256) void emb_take_rows_kernel(const EmbCol c, const uint32_t* __restrict__ idx, uint64_t nout,
                                                            uint8_t* __restrict__ out_validity, unsigned long long* __restrict__ ctrl) {
    const unsigned lane = threadIdx.x & 63;
    EmbCounts counts;
    const uint64_t stride = (uint64_t)gridDim.x * 256, rounds = (nout + stride - 1) / stride;  // uniform: every lane reaches the ballots
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t o = t * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x, base = o - lane;
        const bool mine = o < nout;
        uint64_t start = 0;
        uint32_t state = kRowAbsent;
        uint64_t r = 0;
        if (mine) {
            r = idx[o];
            state = r == OXH_TAKE_NULL ? kRowNull : r >= c.nrows || r < c.row0 ? kRowBadIndex : emb_row(c, r, start);
        }
        const unsigned long long valid = __ballot(state == kRowOk);
        if (lane < 8 && base + 8 * lane < nout) out_validity[(base >> 3) + lane] = (uint8_t)(valid >> (8 * lane));
        counts.add(state, mine, r);
    }
    counts.flush(ctrl, lane);
}

// out[o * dim + d] = element d of row idx[o], 0.0f where that row is absent, null or not read.
__global__ __launch_bounds__(256) void emb_take_values_kernel(const EmbCol c, const uint32_t* __restrict__ idx, uint64_t nout,
                                                              float* __restrict__ out) {
    const uint64_t total = nout * c.dim, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const uint64_t o = e / c.dim, d = e - o * c.dim;
        const uint64_t r = idx[o];
        uint64_t start = 0;
        const bool ok = r != OXH_TAKE_NULL && r < c.nrows && r >= c.row0 && emb_row(c, r, start) == kRowOk;
        out[e] = ok ? c.values[start + d] : 0.0f;
    }
}

}  // namespace oxh

namespace {

namespace emb = oxh::embedding;
using oxh::EmbCol;

int device_enter(oxh_ctx* ctx) {
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

EmbCol device_col(const emb::Column& c) {
    return EmbCol{(const float*)c.values, (const uint8_t*)c.offsets, c.validity, c.validity_bit, 0, 0, c.nrows, c.dim, c.layout};
}

// The column of a host form inside its block: only the rows [plan.row_lo, plan.row_hi) are there.
EmbCol staged_col(const emb::Column& c, const emb::HostPlan& plan, uint8_t* block) {
    return EmbCol{(const float*)plan.at(block, plan.values), plan.at(block, plan.offsets), plan.at(block, plan.validity), plan.nbit,
                  plan.row_lo, plan.elem_lo, c.nrows, c.dim, c.layout};
}

int copy_up(const emb::HostPlan& plan, uint8_t* block, hipStream_t st) {
    for (const emb::Piece& p : plan.pieces)
        if (p.src && p.bytes) HIP_TRY(hipMemcpyAsync(block + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
    return OXH_OK;
}

// The control words of a call: zeroed but the first wrong row, which starts at "none".
int ctrl_reset(unsigned long long* d_ctrl, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(d_ctrl, 0, oxh::kEmbCtrlWords * 8, st));
    HIP_TRY(hipMemsetAsync(d_ctrl + oxh::kEmbCtrlFirstWrong, 0xFF, 8, st));
    return OXH_OK;
}

// stats4 from the control words, and what they make the call return.
int ctrl_verdict(const char* what, const unsigned long long* h_ctrl, uint64_t nrows, uint64_t* stats4) {
    stats4[0] = h_ctrl[oxh::kEmbCtrlUsed], stats4[1] = h_ctrl[oxh::kEmbCtrlNull], stats4[2] = h_ctrl[oxh::kEmbCtrlWrong];
    stats4[3] = h_ctrl[oxh::kEmbCtrlWrong] ? h_ctrl[oxh::kEmbCtrlFirstWrong] : nrows;
    STEP("%s: %llu rows used, %llu null, %llu of another length", what, (unsigned long long)stats4[0], (unsigned long long)stats4[1],
         (unsigned long long)stats4[2]);
    if (h_ctrl[oxh::kEmbCtrlErr] & oxh::kEmbErrIndex) return fail(OXH_ERR_INVALID, std::string(what) + ": an index is not a row of the column (it was not read)");
    if (h_ctrl[oxh::kEmbCtrlErr] & oxh::kEmbErrOffsets)
        return fail(OXH_ERR_INVALID, std::string(what) + ": the offsets of a list column decrease or are negative (those rows were not read)");
    if (stats4[2])
        return fail(OXH_ERR_INVALID, std::string(what) + ": " + std::to_string(stats4[2]) + " valid rows are not of length dim, the first is row " +
                                         std::to_string(stats4[3]) + " (they were not read)");
    return OXH_OK;
}

// One lease for a call's scratch: `bytes` on the device (the control words at its front) and the pinned words
// they come back to.
struct CallScratch {
    oxh::ScratchLease lease;
    uint8_t* base = nullptr;
    unsigned long long* h_ctrl = nullptr;
    explicit CallScratch(hipStream_t st) : lease(st) {}
    int make(uint64_t bytes, const char* what) {
        void *b = nullptr, *p = nullptr;
        if (lease.get(bytes, &b) != hipSuccess || lease.pinned(emb::kCtrlBytes, &p) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, std::string(what) + ": " + std::to_string(bytes) + " B of scratch");
        }
        base = (uint8_t*)b, h_ctrl = (unsigned long long*)p;
        return OXH_OK;
    }
    unsigned long long* d_ctrl() const { return (unsigned long long*)base; }
    int fetch(hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(h_ctrl, base, oxh::kEmbCtrlWords * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }
};

unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), oxh::kEmbGridCap); }

// ---------------------------------------------------------------- mean
int mean_run(const EmbCol& c, const uint32_t* d_idx, uint64_t nidx, float* d_out, uint64_t* stats4, hipStream_t st) {
    const uint32_t groups = emb::mean_groups(nidx), lanes = emb::mean_lanes(c.dim);
    CallScratch scratch(st);  // ends (and waits for the stream) when the call returns
    int rc = scratch.make(emb::mean_lease_bytes(nidx, c.dim), "embedding mean");
    if (rc) return rc;
    float* d_partial = (float*)(scratch.base + emb::kCtrlBytes);
    rc = [&]() -> int {
        int r = ctrl_reset(scratch.d_ctrl(), st);
        if (r) return r;
        if (nidx) {
            oxh::emb_mean_partial_kernel<<<groups, 256, 0, st>>>(c, d_idx, nidx, lanes, d_partial, scratch.d_ctrl());
            HIP_TRY(hipGetLastError());
            oxh::emb_mean_finish_kernel<<<(c.dim + 255) / 256, 256, 0, st>>>(d_partial, groups, c.dim, scratch.d_ctrl(), d_out);
            HIP_TRY(hipGetLastError());
        }
        return scratch.fetch(st);
    }();
    if (rc != OXH_OK) {
        (void)hipStreamSynchronize(st);  // work of a failed call may still be queued
        return rc;
    }
    return ctrl_verdict("embedding mean", scratch.h_ctrl, c.nrows, stats4);
}

int mean_enter(oxh_ctx* ctx, const emb::MeanArgs& a, bool host, bool& done) {
    done = false;
    const std::string what = emb::mean_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "embedding mean: " + what);
    if (a.col.nrows == 0) {
        a.stats4[0] = a.stats4[1] = a.stats4[2] = a.stats4[3] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

// ---------------------------------------------------------------- similarity
template <int LPR>
int similarity_launch(const EmbCol& c, const float* d_query, float* d_sim, uint8_t* d_valid, uint32_t* d_key, unsigned long long* d_ctrl,
                      hipStream_t st) {
    constexpr uint64_t task = LPR == 64 ? 8 : 64;
    const uint64_t ntasks = (c.nrows + task - 1) / task;
    const unsigned grid = (unsigned)std::min<uint64_t>((ntasks + 3) / 4, oxh::kEmbGridCap);
    if (c.dim <= oxh::kEmbQueryLds)
        oxh::emb_similarity_kernel<LPR, true><<<grid, 256, (size_t)c.dim * 4, st>>>(c, d_query, d_sim, d_valid, d_key, d_ctrl);
    else
        oxh::emb_similarity_kernel<LPR, false><<<grid, 256, 0, st>>>(c, d_query, d_sim, d_valid, d_key, d_ctrl);
    HIP_TRY(hipGetLastError());
    return OXH_OK;
}

// sim, the validity bytes and the order keys; the stream has drained on return. The sort is the caller's next step.
int similarity_run(const EmbCol& c, const float* d_query, float* d_sim, uint8_t* d_valid, uint32_t* d_key, uint64_t* stats4, hipStream_t st) {
    CallScratch scratch(st);
    int rc = scratch.make(emb::kCtrlBytes, "embedding similarity");
    if (rc) return rc;
    rc = [&]() -> int {
        int r = ctrl_reset(scratch.d_ctrl(), st);
        if (r) return r;
        r = c.dim <= oxh::kEmbQuadDimMax      ? similarity_launch<4>(c, d_query, d_sim, d_valid, d_key, scratch.d_ctrl(), st)
            : c.dim <= oxh::kEmbSubwaveDimMax ? similarity_launch<16>(c, d_query, d_sim, d_valid, d_key, scratch.d_ctrl(), st)
                                              : similarity_launch<64>(c, d_query, d_sim, d_valid, d_key, scratch.d_ctrl(), st);
        if (r) return r;
        return scratch.fetch(st);
    }();
    if (rc != OXH_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    return ctrl_verdict("embedding similarity", scratch.h_ctrl, c.nrows, stats4);
}

// perm = the stable ascending sort of the order keys: the row sort over that one unsigned 4-byte column. No lease
// is held here; the sort takes its own.
int order_run(oxh_ctx* ctx, uint64_t nrows, const uint32_t* d_key, uint32_t* d_perm, hipStream_t st) {
    const uint32_t kind = OXH_COL_FIXED4, order = OXH_SORT_UNSIGNED;
    const void* values = d_key;
    const void* offsets = nullptr;
    const uint8_t* validity = nullptr;
    const uint64_t bits[2] = {0, 0};
    uint64_t sort_stats[3];
    return oxh_sort_rows_device(ctx, nrows, 1, &kind, &values, &offsets, &validity, bits, &order, d_perm, sort_stats, st);
}

int similarity_enter(oxh_ctx* ctx, const emb::SimilarityArgs& a, bool host, bool& done) {
    done = false;
    const std::string what = emb::similarity_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "embedding similarity: " + what);
    if (a.col.nrows == 0) {
        a.stats4[0] = a.stats4[1] = a.stats4[2] = a.stats4[3] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

// ---------------------------------------------------------------- take
int take_run(const EmbCol& c, const uint32_t* d_idx, uint64_t nout, float* d_out, uint8_t* d_valid, uint64_t* stats4, hipStream_t st) {
    CallScratch scratch(st);
    int rc = scratch.make(emb::kCtrlBytes, "embedding take");
    if (rc) return rc;
    rc = [&]() -> int {
        int r = ctrl_reset(scratch.d_ctrl(), st);
        if (r) return r;
        oxh::emb_take_rows_kernel<<<stride_grid(nout), 256, 0, st>>>(c, d_idx, nout, d_valid, scratch.d_ctrl());
        HIP_TRY(hipGetLastError());
        oxh::emb_take_values_kernel<<<stride_grid(nout * c.dim), 256, 0, st>>>(c, d_idx, nout, d_out);
        HIP_TRY(hipGetLastError());
        return scratch.fetch(st);
    }();
    if (rc != OXH_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    return ctrl_verdict("embedding take", scratch.h_ctrl, c.nrows, stats4);
}

int take_enter(oxh_ctx* ctx, const emb::TakeArgs& a, bool host, bool& done) {
    done = false;
    const std::string what = emb::take_error(a, host);
    if (!what.empty()) return fail(OXH_ERR_INVALID, "embedding take: " + what);
    if (a.nout == 0) {
        a.stats4[0] = a.stats4[1] = a.stats4[2] = a.stats4[3] = 0;
        done = true;
        return OXH_OK;
    }
    return device_enter(ctx);
}

// A host form's block, freed when the call returns.
struct DeviceBlock {
    uint8_t* d = nullptr;
    ~DeviceBlock() {
        if (d) (void)hipFree(d);
    }
    int make(uint64_t bytes, const char* what, hipStream_t st) {
        if (hipMalloc(&d, bytes + 16) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, std::string(what) + ": " + std::to_string(bytes) + " B for the named rows on the device");
        }
        oxh::poison_device(d, bytes + 16, st);
        return OXH_OK;
    }
};

}  // namespace

extern "C" {

int oxh_embedding_mean_device(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* d_values, const void* d_offsets,
                              const uint8_t* d_validity, uint64_t validity_bit, const uint32_t* d_idx, uint64_t nidx, void* d_out,
                              uint64_t* stats4, void* stream) {
    const emb::MeanArgs a{{layout, nrows, dim, d_values, d_offsets, d_validity, validity_bit}, d_idx, nidx, d_out, stats4};
    bool done = false;
    int rc = mean_enter(ctx, a, false, done);
    if (rc || done) return rc;
    return mean_run(device_col(a.col), d_idx, nidx, (float*)d_out, stats4, (hipStream_t)stream);
}

int oxh_embedding_mean_host(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* values, const void* offsets,
                            const uint8_t* validity, uint64_t validity_bit, const uint32_t* idx, uint64_t nidx, void* out,
                            uint64_t* stats4) {
    const emb::MeanArgs a{{layout, nrows, dim, values, offsets, validity, validity_bit}, idx, nidx, out, stats4};
    bool done = false;
    int rc = mean_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // only the rows between the smallest and the largest index are staged (every index is a row: mean_error)
    uint64_t lo = nrows, hi = 0;
    for (uint64_t i = 0; i < nidx; ++i) lo = std::min<uint64_t>(lo, idx[i]), hi = std::max<uint64_t>(hi, (uint64_t)idx[i] + 1);
    emb::HostPlan plan;
    const int64_t p_out = plan.add(nullptr, (uint64_t)dim * 4);
    const int64_t p_idx = plan.add(idx, nidx * 4);
    plan.add_column(a.col, std::min(lo, hi), hi);
    DeviceBlock block;
    if ((rc = block.make(plan.total, "embedding mean", st))) return rc;
    uint64_t stats[4] = {0, 0, 0, 0};
    std::vector<float> mean(dim);
    rc = [&]() -> int {
        int r = copy_up(plan, block.d, st);
        if (r) return r;
        r = mean_run(staged_col(a.col, plan, block.d), (const uint32_t*)plan.at(block.d, p_idx), nidx, (float*)plan.at(block.d, p_out), stats, st);
        if (r) return r;
        if (stats[0]) {
            HIP_TRY(hipMemcpyAsync(mean.data(), plan.at(block.d, p_out), (size_t)dim * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    memcpy(stats4, stats, sizeof stats);
    if (rc) return rc;  // out stays untouched unless everything succeeded
    if (stats[0]) memcpy(out, mean.data(), (size_t)dim * 4);
    return OXH_OK;
}

int oxh_embedding_similarity_device(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* d_values, const void* d_offsets,
                                    const uint8_t* d_validity, uint64_t validity_bit, const void* d_query, void* d_sim,
                                    uint8_t* d_sim_validity, uint32_t* d_order_key, uint32_t* d_perm, uint64_t* stats4, void* stream) {
    const emb::SimilarityArgs a{{layout, nrows, dim, d_values, d_offsets, d_validity, validity_bit}, d_query, d_sim, d_sim_validity, d_order_key,
                                d_perm, stats4};
    bool done = false;
    int rc = similarity_enter(ctx, a, false, done);
    if (rc || done) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = similarity_run(device_col(a.col), (const float*)d_query, (float*)d_sim, d_sim_validity, d_order_key, stats4, st);
    // the keys are complete even where rows were refused (theirs is the null key): the order is given with the error
    if ((rc == OXH_OK || rc == OXH_ERR_INVALID) && d_perm) {
        const std::string said = g_err;
        const int sorted = order_run(ctx, nrows, d_order_key, d_perm, st);
        if (sorted) return sorted;
        g_err = said;
    }
    return rc;
}

int oxh_embedding_similarity_host(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* values, const void* offsets,
                                  const uint8_t* validity, uint64_t validity_bit, const void* query, void* sim, uint8_t* sim_validity,
                                  uint32_t* order_key, uint32_t* perm, uint64_t* stats4) {
    const emb::SimilarityArgs a{{layout, nrows, dim, values, offsets, validity, validity_bit}, query, sim, sim_validity, order_key, perm, stats4};
    bool done = false;
    int rc = similarity_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t bitmap = (nrows + 7) / 8;
    emb::HostPlan plan;
    const int64_t p_sim = plan.add(nullptr, nrows * 4);
    const int64_t p_valid = sim_validity ? plan.add(nullptr, bitmap) : -1;
    const int64_t p_key = order_key ? plan.add(nullptr, nrows * 4) : -1;
    const int64_t p_perm = perm ? plan.add(nullptr, nrows * 4) : -1;
    const int64_t p_query = plan.add(query, (uint64_t)dim * 4);
    plan.add_column(a.col, 0, nrows);
    DeviceBlock block;
    if ((rc = block.make(plan.total, "embedding similarity", st))) return rc;
    uint64_t stats[4] = {0, 0, 0, 0};
    std::vector<uint8_t> back(plan.pieces[p_query].at);  // the outputs stand in front of the query
    rc = [&]() -> int {
        int r = copy_up(plan, block.d, st);
        if (r) return r;
        uint32_t* d_key = (uint32_t*)plan.at(block.d, p_key);
        r = similarity_run(staged_col(a.col, plan, block.d), (const float*)plan.at(block.d, p_query), (float*)plan.at(block.d, p_sim),
                           plan.at(block.d, p_valid), d_key, stats, st);
        if (r) return r;
        if (perm && (r = order_run(ctx, nrows, d_key, (uint32_t*)plan.at(block.d, p_perm), st))) return r;
        HIP_TRY(hipMemcpyAsync(back.data(), block.d, back.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    memcpy(stats4, stats, sizeof stats);
    if (rc) return rc;  // the caller's arrays stay untouched unless everything succeeded
    memcpy(sim, back.data() + plan.pieces[p_sim].at, nrows * 4);
    if (sim_validity) memcpy(sim_validity, back.data() + plan.pieces[p_valid].at, bitmap);
    if (order_key) memcpy(order_key, back.data() + plan.pieces[p_key].at, nrows * 4);
    if (perm) memcpy(perm, back.data() + plan.pieces[p_perm].at, nrows * 4);
    return OXH_OK;
}

int oxh_embedding_take_device(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* d_values, const void* d_offsets,
                              const uint8_t* d_validity, uint64_t validity_bit, const uint32_t* d_idx, uint64_t nout, void* d_out_values,
                              uint8_t* d_out_validity, uint64_t* stats4, void* stream) {
    const emb::TakeArgs a{{layout, nrows, dim, d_values, d_offsets, d_validity, validity_bit}, d_idx, nout, d_out_values, d_out_validity, stats4};
    bool done = false;
    int rc = take_enter(ctx, a, false, done);
    if (rc || done) return rc;
    return take_run(device_col(a.col), d_idx, nout, (float*)d_out_values, d_out_validity, stats4, (hipStream_t)stream);
}

int oxh_embedding_take_host(oxh_ctx* ctx, uint32_t layout, uint64_t nrows, uint32_t dim, const void* values, const void* offsets,
                            const uint8_t* validity, uint64_t validity_bit, const uint32_t* idx, uint64_t nout, void* out_values,
                            uint8_t* out_validity, uint64_t* stats4) {
    const emb::TakeArgs a{{layout, nrows, dim, values, offsets, validity, validity_bit}, idx, nout, out_values, out_validity, stats4};
    bool done = false;
    int rc = take_enter(ctx, a, true, done);
    if (rc || done) return rc;
    hipStream_t st = ctx->stream;
    // only the rows between the smallest and the largest present index are staged (every one is a row: take_error)
    uint64_t lo = nrows, hi = 0;
    for (uint64_t i = 0; i < nout; ++i)
        if (idx[i] != OXH_TAKE_NULL) lo = std::min<uint64_t>(lo, idx[i]), hi = std::max<uint64_t>(hi, (uint64_t)idx[i] + 1);
    const uint64_t bitmap = (nout + 7) / 8, floats = nout * dim;
    emb::HostPlan plan;
    const int64_t p_out = plan.add(nullptr, floats * 4);
    const int64_t p_valid = plan.add(nullptr, bitmap);
    const int64_t p_idx = plan.add(idx, nout * 4);
    plan.add_column(a.col, std::min(lo, hi), hi);
    DeviceBlock block;
    if ((rc = block.make(plan.total, "embedding take", st))) return rc;
    uint64_t stats[4] = {0, 0, 0, 0};
    std::vector<uint8_t> back(plan.pieces[p_idx].at);  // the outputs stand in front of the indices
    rc = [&]() -> int {
        int r = copy_up(plan, block.d, st);
        if (r) return r;
        r = take_run(staged_col(a.col, plan, block.d), (const uint32_t*)plan.at(block.d, p_idx), nout, (float*)plan.at(block.d, p_out),
                     plan.at(block.d, p_valid), stats, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(back.data(), block.d, back.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return OXH_OK;
    }();
    if (rc != OXH_OK) (void)hipStreamSynchronize(st);
    memcpy(stats4, stats, sizeof stats);
    if (rc) return rc;
    memcpy(out_values, back.data() + plan.pieces[p_out].at, floats * 4);
    memcpy(out_validity, back.data() + plan.pieces[p_valid].at, bitmap);
    return OXH_OK;
}

}  // extern "C"
