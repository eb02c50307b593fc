// oxen_amd/csrc/fastcdc.hip -- FastCDC v2020 content-defined chunk boundaries on gfx950
// (block-level dedup), and the chunk digests behind them: the device call
// oxh_fastcdc_device, and the kernels that follow either pipeline.
//
// Reference: experiments/block-level-dedup/src/chunker/fastcdchunker.rs:83-98 calls
// `fastcdc::v2020::FastCDC::new(&content, 4096, chunk, 2 * chunk)` (crate fastcdc 3.2.1, not
// vendored) and names every chunk by the decimal xxh3_128 of its bytes. The crate's cut_gear rolls
// a 64-bit gear hash `h = (h << 1) + GEAR[b]` from index `min` of every chunk and cuts at the first
// position whose hash has no bit of mask_s (before `avg`) or mask_l (after it); else at `max`.
//
// The walk is serial per file (each cut decides where the next chunk's hash starts). Two GPU
// formulations produce per-section lists of chunk starts and the stitch tables over them:
//   fastcdc_scan.hip  F1 scan, F2 speculative walk, F3 stitch: avg > 16 KiB, and wherever the walk's
//                     layout rules fail
//   fastcdc_walk.hip  W (the walk itself, skipping every chunk's `min` bytes) and X (its exact check)
// fastcdc_plan.hpp chooses between them and sizes their sections (host arithmetic, tested on the CPU);
// fastcdc_device.hpp holds what the three files share. Here: a prefix sum over the per-section chunk
// counts, cdc_emit_kernel writes the chunk table, then K1 hashes every chunk
// (oxh_xxh3_128_batch_device).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "env.hpp"
#include "fastcdc_device.hpp"
#include "scratch.hpp"

namespace oxh {

int set_error(int code, const std::string& msg);  // capi_context.hip: oxh_last_error() text
int k1_packed(const void* d_arena, const uint64_t* d_offsets, const uint64_t* d_lens, uint64_t n, uint64_t* d_out,
              uint64_t mean_len, hipStream_t st);  // capi_dispatch.hip

// F3c: exclusive prefix of the per-section counts (one block; n_sec is ~ bytes / 512 KiB). Every
// thread owns a run of `per` counts (a multiple of 4, so the run starts 16-B aligned: count is a
// 256-B aligned scratch part) and sums it with independent 16-byte loads; one load per count, each
// waiting on the one before through the running sum, took 0.43 ms for C5's 262 144 sections.
__global__ __launch_bounds__(1024) void cdc_prefix_kernel(CdcStitch s, uint64_t n_sec) {
    __shared__ uint64_t part[1024];
    const uint64_t per = ((n_sec + 1023) / 1024 + 3) & ~3ull;
    const uint64_t b = (uint64_t)threadIdx.x * per < n_sec ? (uint64_t)threadIdx.x * per : n_sec;
    const uint64_t e = b + per < n_sec ? b + per : n_sec;
    const uint4* __restrict__ c4 = (const uint4*)s.count;
    uint64_t sum = 0, i = b;
#pragma unroll 8
    for (; i + 4 <= e; i += 4) {
        const uint4 v = c4[i >> 2];
        sum += (uint64_t)v.x + v.y + v.z + v.w;
    }
    for (; i < e; ++i) sum += s.count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    // four counts per 16-byte load, four bases per two 16-byte stores (out_base + b is 32-B aligned)
    ulonglong2* __restrict__ o2 = (ulonglong2*)s.out_base;
    i = b;
#pragma unroll 4
    for (; i + 4 <= e; i += 4) {
        const uint4 v = c4[i >> 2];
        const uint64_t r1 = run + v.x, r2 = r1 + v.y, r3 = r2 + v.z;
        o2[i >> 1] = make_ulonglong2(run, r1);
        o2[(i >> 1) + 1] = make_ulonglong2(r2, r3);
        run = r3 + v.w;
    }
    for (; i < e; ++i) {
        s.out_base[i] = run;
        run += s.count[i];
    }
    if (threadIdx.x == 1023) s.out_base[n_sec] = part[1023];
}

// F3d: the chunk table. One lane per chunk start, grouped by section (a wave per section).
__global__ __launch_bounds__(256) void cdc_emit_kernel(CdcFiles f, CdcParams prm, CdcStitch s, uint64_t n_sec,
                                                       uint64_t* __restrict__ c_off, uint64_t* __restrict__ c_len) {
    const uint64_t sec = (uint64_t)blockIdx.x * 4 + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (sec >= n_sec) return;
    const int lane = threadIdx.x & 63;
    const uint32_t file = f.sec_file[sec];
    const uint64_t sec_start = (sec - f.sec_base[file]) * prm.sec;
    const uint64_t foff = f.foff[file];
    const uint32_t cnt = s.count[sec];
    const uint32_t* src = s.status[sec] == kFixed ? s.fix + sec * prm.speccap : f.spec + sec * prm.speccap + s.k0[sec];
    const uint64_t base = s.out_base[sec];
    const uint64_t ex = s.exit[sec];
    for (uint32_t k = lane; k < cnt; k += 64) {
        const uint64_t a = sec_start + src[k];
        const uint64_t b = k + 1 < cnt ? sec_start + src[k + 1] : ex;
        c_off[base + k] = foff + a;
        c_len[base + k] = b - a;
    }
}

// per-file first chunk index
__global__ void cdc_first_kernel(const uint64_t* __restrict__ sec_base, const uint64_t* __restrict__ out_base,
                                 uint64_t n_files, uint64_t* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_files) first[i] = out_base[sec_base[i]];
}

// File of every section (sec_base is the exclusive prefix of per-file section counts): built on the
// device so no section-sized table is copied from pageable host memory.
__global__ void cdc_sec_file_kernel(const uint64_t* __restrict__ sec_base, uint64_t n_files, uint64_t n_sec,
                                    uint32_t* __restrict__ sec_file) {
    const uint64_t sec = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sec >= n_sec) return;
    uint64_t lo = 0, hi = n_files;  // last file with sec_base[file] <= sec
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sec_base[mid] <= sec) lo = mid;
        else hi = mid;
    }
    sec_file[sec] = (uint32_t)lo;
}

}  // namespace oxh

// ---------------------------------------------------------------- host side
namespace {

int cdc_fail(int code, const std::string& msg) { return oxh::set_error(code, msg); }

#define CDC_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return cdc_fail(OXH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Per-call scratch (candidate lists, speculative starts, stitch tables) carved out of the device's
// cached scratch buffer (scratch.hpp).
struct Scratch {
    oxh::ScratchLease lease;
    std::vector<std::pair<void**, uint64_t>> parts;
    explicit Scratch(hipStream_t s) : lease(s) {}
    template <class T>
    void want(T** p, uint64_t count) {
        parts.push_back({(void**)p, (std::max<uint64_t>(count, 1) * sizeof(T) + 255) & ~255ull});
    }
    hipError_t commit() {
        uint64_t total = 0;
        for (auto& q : parts) total += q.second;
        void* base = nullptr;
        const hipError_t e = lease.get(total, &base);
        if (e != hipSuccess) return e;
        uint64_t off = 0;
        for (auto& q : parts) {
            *q.first = (uint8_t*)base + off;
            off += q.second;
        }
        return hipSuccess;
    }
};

}  // namespace

extern "C" {

int oxh_fastcdc_gear(uint64_t* out256) {
    if (!out256) return cdc_fail(OXH_ERR_INVALID, "null output");
    memcpy(out256, oxh::kGear, sizeof(oxh::kGear));
    return OXH_OK;
}

int oxh_fastcdc_masks(uint32_t avg_size, uint32_t level, uint64_t* mask_s, uint64_t* mask_l) {
    // only avg and level matter here: min and max at legal values
    const char* bad = nullptr;
    if (int rc = oxh::cdc_check_params(64, avg_size, 1024, level, &bad)) return cdc_fail(rc, bad);
    uint64_t ms = 0, ml = 0;
    oxh::cdc_masks(avg_size, level, &ms, &ml);
    if (mask_s) *mask_s = ms;
    if (mask_l) *mask_l = ml;
    return OXH_OK;
}

uint64_t oxh_fastcdc_max_chunks(const uint64_t* lens, uint64_t n, uint32_t min_size) {
    uint64_t t = 0;
    for (uint64_t i = 0; i < n; ++i) t += lens[i] ? (lens[i] + min_size - 1) / std::max<uint32_t>(min_size, 1) : 0;
    return t;
}

int oxh_fastcdc_device(const void* d_arena, const uint64_t* offsets, const uint64_t* lens, uint64_t n,
                       uint32_t min_size, uint32_t avg_size, uint32_t max_size, uint32_t level,
                       uint64_t* d_chunk_offsets, uint64_t* d_chunk_lens, uint64_t* d_digests, uint64_t capacity,
                       uint64_t* first_chunk, void* stream) {
    const char* bad = nullptr;
    if (int rc = oxh::cdc_check_params(min_size, avg_size, max_size, level, &bad)) return cdc_fail(rc, bad);
    if (n > 0 && (!d_arena || !offsets || !lens || !first_chunk)) return cdc_fail(OXH_ERR_INVALID, "null argument");
    if (!first_chunk) return cdc_fail(OXH_ERR_INVALID, "null first_chunk");
    hipStream_t st = (hipStream_t)stream;
    first_chunk[0] = 0;
    if (n == 0) return OXH_OK;

    // the plan (fastcdc_plan.hpp): scan or walk, the section geometry, the per-file section table
    int dev = 0, cus = 0, max_lds = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) max_lds = 64 * 1024;
    const oxh::CdcPlanInput in{offsets, lens, n, min_size, avg_size, max_size, level, (uint64_t)(uintptr_t)d_arena, cus, max_lds,
                               oxh::env::cdc_walk(), oxh::env::cdc_section_bytes(), oxh::env::cdc_warmup_bytes(),
                               oxh::env::cdc_unit_cap()};
    oxh::CdcPlan plan;
    if (int rc = oxh::cdc_plan(in, plan)) return cdc_fail(rc, plan.error);
    const oxh::CdcParams& prm = plan.prm;
    const uint64_t n_sec = plan.n_sec;
    const bool walk = plan.walk;

    // OXH_TRACE=1: host-side stage times of this call on stderr
    static const bool trace = oxh::env::trace();
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    Scratch sc(st);
    uint64_t *d_foff, *d_flen, *d_sec_base, *d_first, *d_exit, *d_out_base;
    uint32_t *d_sec_file, *d_spec, *d_spec_cnt, *d_status, *d_k0, *d_count, *d_fix;
    uint64_t* d_cand_occ;
    oxh::CandRec* d_cand;
    sc.want(&d_foff, n);
    sc.want(&d_flen, n);
    sc.want(&d_sec_base, n + 1);
    sc.want(&d_first, n + 1);
    uint32_t* d_entry = nullptr;
    sc.want(&d_sec_file, n_sec);
    if (walk) {
        d_cand = nullptr, d_cand_occ = nullptr;
        sc.want(&d_entry, n_sec);
    } else {
        sc.want(&d_cand, n_sec * 64 * prm.cap);
        sc.want(&d_cand_occ, n_sec);
    }
    sc.want(&d_spec, n_sec * prm.speccap);
    sc.want(&d_spec_cnt, n_sec);
    sc.want(&d_status, n_sec);
    sc.want(&d_k0, n_sec);
    sc.want(&d_count, n_sec);
    sc.want(&d_exit, n_sec);
    sc.want(&d_fix, n_sec * prm.speccap);
    sc.want(&d_out_base, n_sec + 1);
    CDC_HIP(sc.commit());
    const double t_malloc = since();
    CDC_HIP(hipMemcpyAsync(d_foff, offsets, n * 8, hipMemcpyHostToDevice, st));
    CDC_HIP(hipMemcpyAsync(d_flen, lens, n * 8, hipMemcpyHostToDevice, st));
    CDC_HIP(hipMemcpyAsync(d_sec_base, plan.sec_base.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_sec) {
        hipLaunchKernelGGL(oxh::cdc_sec_file_kernel, dim3((unsigned)((n_sec + 255) / 256)), dim3(256), 0, st, d_sec_base, n,
                           n_sec, d_sec_file);
        CDC_HIP(hipGetLastError());
    }

    const double t_alloc = since();
    oxh::CdcFiles f{(const uint8_t*)d_arena, d_foff, d_flen, d_sec_base, d_sec_file, d_cand, d_cand_occ, d_spec, d_spec_cnt};
    oxh::CdcStitch sti{d_status, d_k0, d_count, d_exit, d_fix, d_out_base};
    if (n_sec) {
        // either pipeline leaves the per-section start lists and stitch tables; then the counts' prefix
        if (walk) CDC_HIP(oxh::cdc_launch_walk(f, prm, sti, n_sec, n, plan.arena_bytes, d_entry, st));
        else CDC_HIP(oxh::cdc_launch_scan(f, prm, sti, n_sec, n, st));
        hipLaunchKernelGGL(oxh::cdc_prefix_kernel, dim3(1), dim3(1024), 0, st, sti, n_sec);
        CDC_HIP(hipGetLastError());
    } else {
        CDC_HIP(hipMemsetAsync(d_out_base, 0, 8, st));
    }
    hipLaunchKernelGGL(oxh::cdc_first_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, d_sec_base, d_out_base, n,
                       d_first);
    CDC_HIP(hipGetLastError());
    CDC_HIP(hipMemcpyAsync(first_chunk, d_first, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    const double t_launch = since();
    CDC_HIP(hipStreamSynchronize(st));
    if (trace)
        fprintf(stderr, "[oxh] fastcdc: %s sections=%llu (%llu B, warm-up %llu B) malloc=%.4fs copy=%.4fs launch=%.4fs "
                "chunking=%.4fs scratch=%.2fGiB\n", walk ? "walk" : "scan", (unsigned long long)n_sec,
                (unsigned long long)prm.sec, (unsigned long long)prm.warmup, t_malloc, t_alloc - t_malloc, t_launch - t_alloc,
                since(), sc.lease.size() / 1073741824.0);
    const uint64_t total = first_chunk[n];
    if (total > capacity)
        return cdc_fail(OXH_ERR_INVALID, "chunk capacity too small: need " + std::to_string(total) + " entries");
    if (total && (!d_chunk_offsets || !d_chunk_lens)) return cdc_fail(OXH_ERR_INVALID, "null chunk table");
    if (n_sec) {
        hipLaunchKernelGGL(oxh::cdc_emit_kernel, dim3((unsigned)((n_sec + 3) / 4)), dim3(256), 0, st, f, prm, sti, n_sec,
                           d_chunk_offsets, d_chunk_lens);
        CDC_HIP(hipGetLastError());
    }
    if (d_digests && total) {
        // chunks sit back to back at arbitrary byte offsets: K1R at small chunks, the block-wise K1
        // otherwise (oxh::k1_packed)
        const int rc = oxh::k1_packed(d_arena, d_chunk_offsets, d_chunk_lens, total, d_digests, plan.total_bytes / total, st);
        if (rc) return cdc_fail(rc, std::string("chunk digests: ") + oxh_last_error());
    }
    CDC_HIP(hipStreamSynchronize(st));
    return OXH_OK;
}

}  // extern "C"
