// oxen_amd/csrc/env.hpp -- every OXH_* environment switch the library reads, one accessor each, with
// its default, its clamp and when it is read. No other file of oxen_amd/csrc calls getenv, and the set
// is the table of INTEGRATION.md §6 (tests/test_env_switches.py holds both). An accessor without a
// `static` reads the environment on every call; "latched" ones read it once per process.
// A switch that only selects the losing arm of a measured A/B does not belong here once the A/B is
// decided: the winning value becomes a constant where it is used.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace oxh::env {

inline const char* text(const char* name) { return getenv(name); }  // nullptr when unset
inline long long integer(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e ? atoll(e) : dflt;
}
inline double real(const char* name, double dflt) {
    const char* e = getenv(name);
    return e ? atof(e) : dflt;
}
inline bool flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

// ---------------------------------------------------------------- caller-facing
// OXH_NUM_THREADS: file readers and the worker pool (cf. OXEN_NUM_THREADS, util/concurrency.rs:1-45);
// 0 = unset or not positive, the caller takes the usable CPUs, at most 16. Read when a context (or its
// FastCDC host pipeline) creates its pools.
inline int num_threads() { return (int)std::max<long long>(0, integer("OXH_NUM_THREADS", 0)); }
// OXH_FLUSH_MIB (default 16): the engine seals a partly filled staging slot at this many bytes when the
// next slot is free. Read at context creation.
inline uint64_t flush_bytes() { return (uint64_t)integer("OXH_FLUSH_MIB", 16) << 20; }
// OXH_BIG_PIECE_MIB (default 1024, at least 1): device piece size of K1L, for device buffers, files and
// host buffers larger than a staging slot. Read per call.
inline uint64_t big_piece_bytes() { return (uint64_t)std::max<long long>(1, integer("OXH_BIG_PIECE_MIB", 1024)) << 20; }
// OXH_BIG_FILES (default 4): files larger than a staging slot that share one large-item pipeline
// (device memory: 2 piece buffers of OXH_BIG_PIECE_MIB + 1 KiB per file). Read per call.
inline int big_files() {
    const long long v = integer("OXH_BIG_FILES", 4);
    return v > 0 ? (int)v : 4;
}
// OXH_STREAM_PIECE_MIB (default 16): piece size of the streaming Xxh3. Read when a stream is created.
inline uint64_t stream_piece_bytes() {
    const long long v = integer("OXH_STREAM_PIECE_MIB", 16);
    return (uint64_t)(v > 0 ? v : 16) << 20;
}
// OXH_CDC_PIECE_MIB (default 1024): device piece size of the host chunk entries, before the call's own
// bounds (two minimal segments, at most 3 GiB, whole bounce windows). Read per call.
inline uint64_t cdc_piece_bytes() {
    const long long v = integer("OXH_CDC_PIECE_MIB", 1024);
    return (uint64_t)(v > 0 ? v : 1024) << 20;
}
// OXH_CDC_BOUNCE_MIB (default 64): one pinned bounce buffer (a window of the piece) of the host chunk
// entries, 16..256 MiB, rounded up to a power of two. Latched.
inline uint64_t cdc_bounce_bytes() {
    static const uint64_t v = [] {
        const long long k = integer("OXH_CDC_BOUNCE_MIB", 64);
        uint64_t m = 16;
        while (m < 256 && (long long)m < k) m <<= 1;
        return m << 20;
    }();
    return v;
}
// OXH_CDC_NBOUNCE (default 8, 2..16): the host chunk entries' ring of bounce buffers; reads of the next
// windows run while earlier H2Ds drain (8: 47.7 vs 43.6 GiB/s for 4 on 16 x 1 GiB from the page cache,
// profiles/r05/r05a_e2e_*). Latched.
constexpr int kCdcNBounceMax = 16;
inline int cdc_nbounce() {
    static const int v = (int)std::max<long long>(2, std::min<long long>(integer("OXH_CDC_NBOUNCE", 8), kCdcNBounceMax));
    return v;
}
// OXH_SCRATCH_KEEP_MIB (default 16384): a device's cached scratch buffer (scratch.hpp) is freed on
// release only when it is larger than this. Latched.
inline uint64_t scratch_keep_bytes() {
    static const uint64_t v = (uint64_t)integer("OXH_SCRATCH_KEEP_MIB", 16384) << 20;
    return v;
}
// OXH_HELPER: the reader-pool helper executable (default: oxh_hash_helper next to this library). Read
// when a pool is created.
inline const char* helper() { return text("OXH_HELPER"); }
// OXH_RCCL_LIB: the RCCL library oxh_comm_* opens before librccl.so.1. Read once, when RCCL is opened.
inline const char* rccl_lib() { return text("OXH_RCCL_LIB"); }
// OXH_GATHER_P2P=1: oxh_gather_digests takes the grouped point-to-point form even for equal shares (the
// ragged path on a one-GPU box). Read per call.
inline bool gather_p2p() { return flag("OXH_GATHER_P2P", false); }
// OXH_WAIT_LIMIT_S (default 60): after this many seconds a wait for GPU work reports which stage never
// finished instead of blocking forever (a staged batch, an engine run, a file request), and a silent
// reader-pool helper is reported on stderr. Read here on every call: the in-process waits latch it at
// their first use, the reader pool reads it per call.
inline double wait_limit_s() { return real("OXH_WAIT_LIMIT_S", 60.0); }
// OXH_POOL_CALL_LIMIT_S (default 0 = none): a deadline for a reader-pool helper's reply; the call then
// fails and the pool is marked unusable. Read per call.
inline double pool_call_limit_s() { return real("OXH_POOL_CALL_LIMIT_S", 0.0); }
// OXH_PUBLISH_INLINE=1: oxh_add_files publishes inside commit() instead of on the committer thread (the
// r02 form). OXH_PUBLISH_SYNC=fsync: the reference's own per-blob steps (fsync the temp, rename, fsync
// its parent) instead of two syncfs barriers per slot, for filesystems where syncfs is costly (one
// shared with other tenants' dirty data). Both read per oxh_add_files call.
inline bool publish_inline() { return flag("OXH_PUBLISH_INLINE", false); }
inline bool publish_fsync() {
    const char* e = text("OXH_PUBLISH_SYNC");
    return e && !strcmp(e, "fsync");
}
// OXH_DIRECT_FILES=0: small file requests on an idle context go to the engine instead of running on
// the caller's thread (A/B, and the tests that compare both forms). Read per call.
inline bool direct_files() { return flag("OXH_DIRECT_FILES", true); }
// OXH_K1_WG_WAVES (1, 2 or 4; else 0 = the library's choice): waves (items) per K1 workgroup on
// descriptor batches, overriding the default and the caller's choice for A/B. Read per launch.
inline int k1_wg_waves() {
    const long long e = integer("OXH_K1_WG_WAVES", 0);
    return (e == 1 || e == 2 || e == 4) ? (int)e : 0;
}
// OXH_CDC_WALK: -1 unset (the walk W + X at avg <= 16 KiB where its layout rules hold), 0 the scan
// F1-F3 always, 1 the walk always (the call fails where a rule does not hold). Read per call.
inline int cdc_walk() {
    const char* e = text("OXH_CDC_WALK");
    return !e ? -1 : atoi(e) != 0 ? 1 : 0;
}

// ---------------------------------------------------------------- host-behaviour escapes
// What library threads do to the process beyond hashing; a host may need these off for reasons a
// benchmark does not see.
// OXH_SHARED_FDS=1: the streaming readers keep the process's file-descriptor table instead of taking
// private ones (unshare(CLONE_FILES), pool.hpp). Read by each reader thread as it starts.
inline bool shared_fds() { return flag("OXH_SHARED_FDS", false); }
// OXH_SPLIT_READS=0: one pread per file; no parts of 4 MiB read by several readers, which reopen the
// first reader's descriptor through /proc (engine.hip). Latched.
inline bool split_reads() {
    static const bool on = flag("OXH_SPLIT_READS", true);
    return on;
}

// ---------------------------------------------------------------- diagnostics and test hooks, not for callers
// OXH_TRACE (set = on): per-call stage times on stderr (host-side wall clock). Read here on every call:
// the host-buffer, engine and large-item calls and a publisher read it per call, the FastCDC entries
// latch it at their first call.
inline bool trace() { return text("OXH_TRACE") != nullptr; }
// OXH_DEBUG_STEPS (set = on): one stderr line per runtime step (locating stalls without a debugger).
// Read once, when the library is loaded (capi_internal.hpp g_steps).
inline bool debug_steps() { return text("OXH_DEBUG_STEPS") != nullptr; }
// Tests of oxh_fastcdc_device, read per call, -1 = unset: OXH_CDC_SECTION_BYTES (many small sections
// per file; the caller takes whole KiB up to 1 GiB, and a set value turns the section sizing off),
// OXH_CDC_WARMUP_BYTES (the speculative walks' warm-up), OXH_CDC_UNIT_CAP (candidates stored per list
// unit, at least 1: forces overflow).
inline long long cdc_section_bytes() { return integer("OXH_CDC_SECTION_BYTES", -1); }
inline long long cdc_warmup_bytes() { return integer("OXH_CDC_WARMUP_BYTES", -1); }
inline int cdc_unit_cap() {
    const char* e = text("OXH_CDC_UNIT_CAP");
    return e ? std::max(1, atoi(e)) : -1;
}

}  // namespace oxh::env
