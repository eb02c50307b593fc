// oxen_amd/csrc/snappy_wave.hpp -- what the Snappy kernels and the Zstandard inflate share (snappy_inflate.hip,
// snappy_compress.hip, zstd_inflate.hip): the order of a wave's LDS and global operations and the whole-wave span copy
// with aligned 16-byte stores.
#pragma once

#include "xxh3_device.hpp"

namespace oxh {

// The LDS of these kernels is private to a wave, whose LDS operations execute in order: the fences only keep the
// compiler from moving them across.
__device__ __forceinline__ void snp_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave's global stores so far are visible to its loads from here on.
__device__ __forceinline__ void snp_global_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Exactly n bytes by the 64 lanes: the bytes up to the destination's 16-byte grid a lane each, then 16 bytes a lane
// (any source alignment, aligned stores), then the last bytes a lane each. ZERO: zeros, src is not read.
template <bool ZERO>
__device__ __forceinline__ void snp_span_wave(uint8_t* dst, const uint8_t* src, uint64_t n, unsigned lane) {
    uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    if (lane < head) dst[lane] = ZERO ? (uint8_t)0 : src[lane];
    const uint64_t body = (n - head) & ~15ull;
    for (uint64_t b = head + 16ull * lane; b < head + body; b += 16ull * 64) {
        ulonglong2 v{0, 0};
        if (!ZERO) v.x = ld64u(src + b), v.y = ld64u(src + b + 8);
        *reinterpret_cast<ulonglong2*>(dst + b) = v;
    }
    const uint64_t tail = head + body;
    if (tail + lane < n) dst[tail + lane] = ZERO ? (uint8_t)0 : src[tail + lane];
}

}  // namespace oxh
