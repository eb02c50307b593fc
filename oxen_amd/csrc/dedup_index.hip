// oxen_amd/csrc/dedup_index.hip -- the device-resident dedup index (oxh_dedup_index_*): which row first
// carried each chunk digest. The block-level-dedup experiment decides that through the file system, one
// stat or file creation per chunk (fixedsize.rs:78-89, fastcdchunker.rs:95-108); here it is a hash
// table in HBM keyed by the 128-bit digests, persistent across calls (DESIGN.md §4 "Dedup index").
//
// State of one index (plain hipMalloc):
//   keys[2r], keys[2r+1] = (lo, hi) of every row ever inserted, by its ordinal r (rows inserted before
//                          the call + the row's position in it);
//   table[slots]           slots a power of two, each an ordinal or EMPTY (~0). The sentinel lives in the
//                          slot, never in a key: digests (0,0) and (~0,~0) are ordinary keys.
// An insert is two launches on one stream, after the call's digests were copied behind the key store:
//   insert   one lane per row: linear probe from lo & mask; an EMPTY slot is claimed with a CAS, a slot
//            of an equal key is lowered to the row's ordinal with an atomic min, any other is passed
//            (a row that repeats the row before it in its wave has nothing to add and returns);
//   resolve  (every min of the insert has landed) each row probes again to the slot of its key and reads
//            the smallest ordinal there; the call's statistics are summed per wave, then per workgroup,
//            one atomic add each (a grid-stride launch, so a few thousand adds in all).
// No lane ever waits for another: a slot's key never changes once claimed (the min only swaps in an
// ordinal of an equal key), so there is nothing to publish and nothing to spin on. Probe loops are
// bounded by the slot count and by the ordinals the table may hold; a lane that runs out sets the
// error word, which the host turns into OXH_ERR_HIP. The host keeps the load at or below one half.
//
// oxh_chunk_overlap_* (how many chunks the versions of a file share, oxendedup.rs:56-70) are here too:
// one insert into a private index gives every digest an id, and two more kernels mark which sets hold
// each id and count the shared rows and bytes of every pair of sets (see at overlap_mark_kernel).
#include "capi_internal.hpp"

using namespace oxh::capi;

namespace oxh {

constexpr unsigned long long kDedupEmpty = ~0ull;
constexpr unsigned long long kErrProbe = 1, kErrOrdinal = 2, kErrMissing = 4;

__device__ __forceinline__ unsigned long long slot_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows [base, base + n) of the key store into `table`; every ordinal the table may hold is below
// `limit` = base + n. With base = 0 this is the re-insert of everything into a fresh table (growth).
// The relaxed loads are hints that spare atomics on one address when many rows carry one key (the
// chunks of a zero-filled file): a slot seen non-EMPTY stays claimed by that key, and slot values only
// fall, among equal keys, so a stale value is still a valid proof. The CAS and the min decide.
__global__ __launch_bounds__(256) void dedup_insert_kernel(const uint64_t* __restrict__ keys, uint64_t base, uint64_t n,
                                                           unsigned long long* __restrict__ table, uint64_t mask,
                                                           unsigned long long* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const uint64_t r = base + i, limit = base + n;
    const uint64_t lo = live ? keys[2 * r] : 0, hi = live ? keys[2 * r + 1] : 0;
    // A row whose key equals that of the row before it can never be the smallest ordinal of its key, and
    // the row before it (or the head of their run) is inserted by this launch: it has nothing to add.
    // Within a wave the neighbour's key is one shuffle away, so a run of equal rows -- a zero-filled
    // region -- puts one probe per wave on its slot instead of 64 (13.1 M equal rows: 6.0 -> 0.20 ms,
    // DESIGN.md §4). Every lane of the wave takes part in the shuffles; nothing returns before them.
    const uint64_t lo_before = (uint64_t)__shfl_up((long long)lo, 1, 64), hi_before = (uint64_t)__shfl_up((long long)hi, 1, 64);
    if (!live || ((threadIdx.x & 63) != 0 && lo_before == lo && hi_before == hi)) return;
    uint64_t slot = lo & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
        unsigned long long j = slot_load(&table[slot]);
        if (j == kDedupEmpty) {
            unsigned long long expected = kDedupEmpty;
            if (__hip_atomic_compare_exchange_strong(&table[slot], &expected, (unsigned long long)r, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                return;
            j = expected;  // another row claimed it first
        }
        if (j >= limit) {  // not an ordinal of this index: never index the key store with it
            __hip_atomic_fetch_or(err, kErrOrdinal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (keys[2 * j] == lo && keys[2 * j + 1] == hi) {
            if (j > r && slot_load(&table[slot]) > r)
                __hip_atomic_fetch_min(&table[slot], (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    __hip_atomic_fetch_or(err, kErrProbe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// first[i] = the ordinal in the slot of q[2i..2i+1]'s key, or ~0 when the probe reaches EMPTY (a query of
// an absent key). INSERTED: the rows are the call's own (ordinals base + i, so none is absent) and the
// call's statistics go to stats[0..3] = {new distinct rows, their bytes, duplicate rows, their bytes}.
template <bool INSERTED>
__global__ __launch_bounds__(256) void dedup_resolve_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ q,
                                                            const uint64_t* __restrict__ lens, uint64_t base, uint64_t n,
                                                            uint64_t limit, const unsigned long long* __restrict__ table,
                                                            uint64_t mask, uint64_t* __restrict__ first,
                                                            unsigned long long* __restrict__ stats,
                                                            unsigned long long* __restrict__ err) {
    // grid-stride over the rows, so that the statistics cost a few thousand atomics whatever n is: one
    // atomic per wave of a row-per-lane grid is 0.8 M adds on one cache line for 13.1 M rows, which that
    // line serves at ~88 per microsecond -- 9 of the 10.6 ms such a launch took
    uint64_t rows_new = 0, rows_dup = 0, bytes_new = 0, bytes_dup = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        unsigned long long found = kDedupEmpty;
        const uint64_t lo = q[2 * i], hi = q[2 * i + 1];
        uint64_t slot = lo & mask;
        unsigned long long bad = kErrProbe;
        for (uint64_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
            const unsigned long long j = table[slot];
            if (j == kDedupEmpty) {
                bad = INSERTED ? kErrMissing : 0;
                break;
            }
            if (j >= limit) {
                bad = kErrOrdinal;
                break;
            }
            if (keys[2 * j] == lo && keys[2 * j + 1] == hi) {
                found = j;
                bad = 0;
                break;
            }
        }
        if (bad) __hip_atomic_fetch_or(err, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (first) first[i] = found;
        if constexpr (INSERTED) {
            const uint64_t len = lens ? lens[i] : 0;
            const bool is_new = found == base + i;
            rows_new += is_new;
            rows_dup += !is_new;
            bytes_new += is_new ? len : 0;
            bytes_dup += is_new ? 0 : len;
        }
    }
    if constexpr (INSERTED) {
        // every lane is here (nothing above returns): wave reduction, the workgroup's four waves summed
        // through LDS, then one 64-bit add per statistic and workgroup. Integer sums: exact, order-free.
        __shared__ unsigned long long part[4][4];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            rows_new += (uint64_t)__shfl_xor((long long)rows_new, off, 64);
            rows_dup += (uint64_t)__shfl_xor((long long)rows_dup, off, 64);
            bytes_new += (uint64_t)__shfl_xor((long long)bytes_new, off, 64);
            bytes_dup += (uint64_t)__shfl_xor((long long)bytes_dup, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* mine = part[threadIdx.x >> 6];
            mine[0] = rows_new, mine[1] = bytes_new, mine[2] = rows_dup, mine[3] = bytes_dup;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
            if (sum) atomicAdd(&stats[threadIdx.x], sum);
        }
    }
}

// ---------------------------------------------------------------- chunk overlap between sets (oxh_chunk_overlap_*)
// The rows are cut into contiguous sets (the chunk tables of a file's versions); first[] of one insert of
// all of them gives every digest an id, the smallest ordinal that carries it. member[id * W + s / 64]
// bit s % 64 = "set s holds this digest" (mark); a later launch (count), so every OR has landed, reads
// the W words of each row's id and adds the row, and its length, to (its set, every set bit). Both
// launch on a (workgroups, nsets) grid: a workgroup works on `chunk` contiguous rows of ONE set, the
// set being blockIdx.y, and leaves at once when its set has no such rows. No lane waits for another.
constexpr unsigned long long kErrFirst = 8, kErrSetBit = 16;
constexpr uint32_t kOverlapMaxSets = OXH_CHUNK_OVERLAP_MAX_SETS;

__global__ __launch_bounds__(256) void overlap_mark_kernel(const uint64_t* __restrict__ first,
                                                           const uint64_t* __restrict__ set_first, uint32_t words, uint64_t n,
                                                           uint64_t chunk, unsigned long long* __restrict__ member,
                                                           unsigned long long* __restrict__ err) {
    const uint32_t s = blockIdx.y;
    const uint64_t lo = set_first[s], rows = set_first[s + 1] - lo, off = (uint64_t)blockIdx.x * chunk;
    if (off >= rows) return;  // the whole workgroup
    const uint64_t end = lo + (rows - off < chunk ? rows : off + chunk);
    const unsigned long long bit = 1ull << (s & 63);
    for (uint64_t at = lo + off; at < end; at += 256) {  // uniform over the workgroup: every lane reaches the shuffle
        const uint64_t i = at + threadIdx.x;
        const bool live = i < end;
        const uint64_t f = live ? first[i] : kDedupEmpty;
        // hints, as in the insert: a lane whose id is that of its wave neighbour (same set: the workgroup
        // has one) has nothing to add, and a bit seen set stays set. The OR decides.
        const uint64_t f_before = (uint64_t)__shfl_up((long long)f, 1, 64);
        if (!live || ((threadIdx.x & 63) != 0 && f_before == f)) continue;
        if (f >= n) {  // not an ordinal of this call: never index the membership array with it
            __hip_atomic_fetch_or(err, kErrFirst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        unsigned long long* p = &member[f * words + (s >> 6)];
        if (!(slot_load(p) & bit)) __hip_atomic_fetch_or(p, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// matrix[a * nsets + b] += rows of set a whose digest set b holds; matrix[nsets^2 + ...] += their lengths.
// Every row of a workgroup belongs to set a and neighbouring rows are mostly in the same sets (bit a at the
// least), so the sums are taken per wave and distinct membership word -- a ballot for the rows, a shuffle
// sum for the lengths -- and added to the workgroup's 2 x nsets counters in LDS; at the end each non-zero
// counter costs one global atomic. Integer sums: exact, order-free.
__global__ __launch_bounds__(256) void overlap_count_kernel(const uint64_t* __restrict__ first, const uint64_t* __restrict__ lens,
                                                            const uint64_t* __restrict__ set_first, uint32_t nsets, uint32_t words,
                                                            uint64_t n, uint64_t chunk,
                                                            const unsigned long long* __restrict__ member,
                                                            unsigned long long* __restrict__ matrix,
                                                            unsigned long long* __restrict__ err) {
    __shared__ unsigned long long cnt[2 * kOverlapMaxSets];
    const uint32_t a = blockIdx.y;
    const uint64_t lo = set_first[a], rows = set_first[a + 1] - lo, off = (uint64_t)blockIdx.x * chunk;
    if (off >= rows) return;  // the whole workgroup, before any barrier
    const uint64_t end = lo + (rows - off < chunk ? rows : off + chunk);
    for (uint32_t k = threadIdx.x; k < 2 * nsets; k += 256) cnt[k] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63;
    for (uint64_t at = lo + off; at < end; at += 256) {  // uniform over the workgroup
        const uint64_t i = at + threadIdx.x;
        bool live = i < end;
        const uint64_t f = live ? first[i] : 0;
        const uint64_t len = live && lens ? lens[i] : 0;
        if (live && f >= n) {
            __hip_atomic_fetch_or(err, kErrFirst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            live = false;
        }
        for (uint32_t w = 0; w < words; ++w) {
            unsigned long long m = live ? member[f * words + w] : 0;
            // each turn takes the word of the first lane that still holds one and serves every lane with that
            // same word: at most 64 turns, and one where a wave's rows are in the same sets. Lane j then adds
            // the turn's rows and bytes for bit j, so the adds of a turn go to different counters.
            for (int turn = 0; turn < 64; ++turn) {
                const unsigned long long pending = __ballot(m != 0);
                if (!pending) break;  // uniform over the wave
                const unsigned long long theirs = (unsigned long long)__shfl((long long)m, __builtin_ctzll(pending), 64);
                const bool same = m == theirs;  // theirs is not 0
                const unsigned long long who = __ballot(same);
                unsigned long long bytes = same ? len : 0;
                if (lens) {
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) bytes += (unsigned long long)__shfl_xor((long long)bytes, o, 64);
                }
                if (same) m = 0;
                if ((theirs >> lane) & 1) {
                    const uint32_t set_b = w * 64 + lane;
                    if (set_b >= nsets) {  // no set of this call: never index the counters with it
                        __hip_atomic_fetch_or(err, kErrSetBit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else {
                        atomicAdd(&cnt[set_b], (unsigned long long)__popcll(who));
                        if (bytes) atomicAdd(&cnt[nsets + set_b], bytes);
                    }
                }
            }
        }
    }
    __syncthreads();
    const uint64_t cells = (uint64_t)nsets * nsets;
    for (uint32_t k = threadIdx.x; k < 2 * nsets; k += 256)
        if (cnt[k]) atomicAdd(&matrix[(k < nsets ? 0 : cells - nsets) + (uint64_t)a * nsets + k], cnt[k]);
}

}  // namespace oxh

namespace {

constexpr uint32_t kMagic = 0x58444944;           // "DIDX": the handle is a void*, so check what it points at
constexpr uint64_t kDefaultRows = 1ull << 16;     // capacity_rows == 0
constexpr uint64_t kMaxRows = 1ull << 40;         // one lane per row in 256-lane workgroups: the grid fits 32 bits
constexpr uint64_t kPieceRows = 1ull << 20;       // host forms: rows per staged piece (32 B of pinned memory each)

struct DedupIndex {
    uint32_t magic = kMagic;
    oxh_ctx* ctx = nullptr;
    int device = 0;
    std::mutex mu;
    bool broken = false;  // a call failed after it had begun to change the table
    uint64_t* d_keys = nullptr;
    uint64_t key_cap = 0;  // rows the key store holds
    unsigned long long* d_table = nullptr;
    uint64_t slots = 0;
    uint64_t rows = 0;
    uint64_t life[4] = {0, 0, 0, 0};          // {rows, distinct, bytes, distinct bytes}
    unsigned long long* d_ctrl = nullptr;     // [0..3] a call's statistics, [4] the error word
    unsigned long long* h_ctrl = nullptr;     // pinned, 8 words
    // host forms: one staged piece, pinned and on the device: [digests 2P | lens P | first P]
    uint64_t* h_piece = nullptr;
    uint64_t* d_piece = nullptr;
};

DedupIndex* as_index(void* p) {
    DedupIndex* ix = static_cast<DedupIndex*>(p);
    return ix && ix->magic == kMagic ? ix : nullptr;
}

uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 2;
    while (p < x) p <<= 1;
    return p;
}

unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }
// resolve: grid-stride, at most 8 workgroups (32 waves, the most 18-20 VGPRs allow) on each of 256 CUs
unsigned resolve_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 2048); }

int error_word(DedupIndex* ix, const char* what) {
    const unsigned long long e = ix->h_ctrl[4];
    if (!e) return OXH_OK;
    ix->broken = true;
    std::string m = std::string(what) + ": ";
    if (e & oxh::kErrProbe) m += "a probe ran through every slot (the table is over its load limit); ";
    if (e & oxh::kErrOrdinal) m += "a slot holds a value that is no ordinal of this index; ";
    if (e & oxh::kErrMissing) m += "an inserted row was not found in the table; ";
    return fail(OXH_ERR_HIP, m + "the index is unusable");
}

// Make room for `n` more rows: a key store of at least rows + n, and a table that stays at or below a
// load of one half. Both new allocations are made before anything changes, so a failed one leaves the
// index as it was (OXH_ERR_NOMEM). `rebuilt` = the table is fresh and empty: the caller re-inserts
// every row.
int reserve(DedupIndex* ix, uint64_t n, hipStream_t st, bool& rebuilt, uint64_t*& old_keys, unsigned long long*& old_table) {
    rebuilt = false;
    old_keys = nullptr;
    old_table = nullptr;
    const uint64_t need = ix->rows + n;
    uint64_t* nk = nullptr;
    unsigned long long* nt = nullptr;
    uint64_t ncap = ix->key_cap, nslots = ix->slots;
    if (need > ix->key_cap) {
        ncap = std::max(need, 2 * ix->key_cap);
        if (hipMalloc(&nk, ncap * 16) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "dedup index: key store of " + std::to_string(ncap) + " rows");
        }
    }
    if (2 * need > ix->slots) {
        nslots = std::max(pow2_at_least(2 * need), 2 * ix->slots);
        if (hipMalloc(&nt, nslots * 8) != hipSuccess) {
            (void)hipGetLastError();
            if (nk) (void)hipFree(nk);
            return fail(OXH_ERR_NOMEM, "dedup index: table of " + std::to_string(nslots) + " slots");
        }
    }
    oxh::poison_device(nk, ncap * 16, st), oxh::poison_device(nt, nslots * 8, st);  // (a NULL one is skipped)
    if (nk) {
        if (ix->rows) HIP_TRY(hipMemcpyAsync(nk, ix->d_keys, ix->rows * 16, hipMemcpyDeviceToDevice, st));
        old_keys = ix->d_keys;
        ix->d_keys = nk;
        ix->key_cap = ncap;
    }
    if (nt) {
        HIP_TRY(hipMemsetAsync(nt, 0xFF, nslots * 8, st));
        old_table = ix->d_table;
        ix->d_table = nt;
        ix->slots = nslots;
        rebuilt = true;
    }
    return OXH_OK;
}

// One insert of n rows whose digests are at `src` (device memory, or pinned host memory: `kind`),
// complete on return. Room is made for `room` >= n rows (a host call's first piece makes it for the
// whole call, so OXH_ERR_NOMEM can only come before any of its rows is in). add4 (may be NULL) is
// incremented by the call's statistics.
int insert_rows(DedupIndex* ix, const uint64_t* src, hipMemcpyKind kind, const uint64_t* d_lens, uint64_t n, uint64_t room,
                uint64_t* d_first, uint64_t* add4, hipStream_t st) {
    if (room > kMaxRows || ix->rows + room > kMaxRows) return fail(OXH_ERR_INVALID, "dedup index: more than 2^40 rows");
    bool rebuilt = false;
    uint64_t* old_keys = nullptr;
    unsigned long long* old_table = nullptr;
    int rc = reserve(ix, room, st, rebuilt, old_keys, old_table);
    if (rc == OXH_OK) {
        ix->broken = true;  // until the call is through: the table may hold ordinals of rows not yet counted
        rc = [&]() -> int {
            const uint64_t base = ix->rows, mask = ix->slots - 1;
            HIP_TRY(hipMemcpyAsync(ix->d_keys + 2 * base, src, n * 16, kind, st));
            HIP_TRY(hipMemsetAsync(ix->d_ctrl, 0, 8 * sizeof(unsigned long long), st));
            if (rebuilt)  // growth: everything, the call's rows included, into the fresh table
                oxh::dedup_insert_kernel<<<grid_for(base + n), 256, 0, st>>>(ix->d_keys, 0, base + n, ix->d_table, mask,
                                                                             ix->d_ctrl + 4);
            else
                oxh::dedup_insert_kernel<<<grid_for(n), 256, 0, st>>>(ix->d_keys, base, n, ix->d_table, mask, ix->d_ctrl + 4);
            HIP_TRY(hipGetLastError());
            oxh::dedup_resolve_kernel<true><<<resolve_grid(n), 256, 0, st>>>(ix->d_keys, ix->d_keys + 2 * base, d_lens, base, n,
                                                                         base + n, ix->d_table, mask, d_first, ix->d_ctrl,
                                                                         ix->d_ctrl + 4);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ix->h_ctrl, ix->d_ctrl, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return OXH_OK;
        }();
    }
    if (old_keys || old_table) {  // the copies out of them were on `st`
        if (rc != OXH_OK) (void)hipStreamSynchronize(st);
        if (old_keys) (void)hipFree(old_keys);
        if (old_table) (void)hipFree(old_table);
    }
    if (rc != OXH_OK) {
        if (rc != OXH_ERR_NOMEM) ix->broken = true;  // OXH_ERR_NOMEM: nothing had changed yet
        return rc;
    }
    if ((rc = error_word(ix, "oxh_dedup_index_insert")) != OXH_OK) return rc;
    ix->broken = false;
    ix->rows += n;
    const uint64_t s[4] = {ix->h_ctrl[0], ix->h_ctrl[1], ix->h_ctrl[2], ix->h_ctrl[3]};
    ix->life[0] += s[0] + s[2];
    ix->life[1] += s[0];
    ix->life[2] += s[1] + s[3];
    ix->life[3] += s[1];
    if (add4)
        for (int k = 0; k < 4; ++k) add4[k] += s[k];
    return OXH_OK;
}

int query_rows(DedupIndex* ix, const uint64_t* d_digests, uint64_t n, uint64_t* d_first, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(ix->d_ctrl, 0, 8 * sizeof(unsigned long long), st));
    oxh::dedup_resolve_kernel<false><<<resolve_grid(n), 256, 0, st>>>(ix->d_keys, d_digests, nullptr, 0, n, ix->rows, ix->d_table,
                                                                  ix->slots - 1, d_first, ix->d_ctrl, ix->d_ctrl + 4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ix->h_ctrl, ix->d_ctrl, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return error_word(ix, "oxh_dedup_index_query");
}

int enter(DedupIndex* ix) {
    if (ix->broken) return fail(OXH_ERR_HIP, "dedup index: an earlier call failed part-way; the index is unusable");
    HIP_TRY(hipSetDevice(ix->device));
    return OXH_OK;
}

int piece_buffers(DedupIndex* ix) {
    if (ix->h_piece) return OXH_OK;
    uint64_t *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, kPieceRows * 32, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OXH_ERR_NOMEM, "dedup index: pinned staging");
    }
    if (hipMalloc(&d, kPieceRows * 32) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(h);
        return fail(OXH_ERR_NOMEM, "dedup index: device staging");
    }
    oxh::poison_pinned(h, kPieceRows * 32), oxh::poison_device(d, kPieceRows * 32, ix->ctx->stream);
    ix->h_piece = h;
    ix->d_piece = d;
    return OXH_OK;
}

// ---------------------------------------------------------------- chunk overlap
// What both forms check before they need a device (the order oxh_dedup_index_create keeps).
int overlap_arguments(const uint64_t* digests, const uint64_t* lens, const uint64_t* set_first, uint64_t nsets,
                      const uint64_t* rows_out, const uint64_t* bytes_out) {
    if (!set_first || !rows_out) return fail(OXH_ERR_INVALID, "chunk overlap: set_first or rows_out is NULL");
    if (nsets == 0 || nsets > OXH_CHUNK_OVERLAP_MAX_SETS)
        return fail(OXH_ERR_INVALID, "chunk overlap: nsets must be 1.." + std::to_string(OXH_CHUNK_OVERLAP_MAX_SETS));
    if (set_first[0] != 0) return fail(OXH_ERR_INVALID, "chunk overlap: set_first[0] is not 0");
    for (uint64_t k = 0; k < nsets; ++k)
        if (set_first[k + 1] < set_first[k]) return fail(OXH_ERR_INVALID, "chunk overlap: set_first decreases at set " + std::to_string(k));
    if (set_first[nsets] > kMaxRows) return fail(OXH_ERR_INVALID, "chunk overlap: more than 2^40 rows");
    if (!digests && set_first[nsets]) return fail(OXH_ERR_INVALID, "chunk overlap: digests is NULL");
    if (bytes_out && !lens) return fail(OXH_ERR_INVALID, "chunk overlap: bytes_out needs the rows' lengths");
    return OXH_OK;
}

// One call's temporaries, all made before any work starts: a private index sized for the rows (so its one
// insert neither grows nor allocates), and one device block
//   [first n | lens n (host form with lengths) | member n*words | matrix 2*nsets^2 | error word | set_first nsets+1]
// with the pinned words the last three cross the link in. Freed once the stream has drained.
struct Overlap {
    DedupIndex* ix = nullptr;
    uint64_t n = 0, nsets = 0, words = 0, cells = 0;
    uint64_t* d_block = nullptr;
    uint64_t *d_first = nullptr, *d_lens = nullptr, *d_sets = nullptr;
    unsigned long long *d_member = nullptr, *d_matrix = nullptr;  // the error word follows the matrix
    uint64_t* h_block = nullptr;  // [matrix 2*nsets^2 | error word | set_first nsets+1]

    int make(oxh_ctx* ctx, const uint64_t* set_first, uint64_t nsets_, bool own_lens, hipStream_t st) {
        nsets = nsets_;
        n = set_first[nsets];
        words = (nsets + 63) / 64;
        cells = nsets * nsets;
        void* handle = nullptr;
        int rc = oxh_dedup_index_create(ctx, n, &handle);
        if (rc) return rc;
        ix = as_index(handle);
        const uint64_t tail = 2 * cells + 1 + nsets + 1;
        if (hipMalloc(&d_block, (n * (1 + (own_lens ? 1 : 0) + words) + tail) * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "chunk overlap: " + std::to_string(n) + " rows of first ordinals and set masks");
        }
        if (hipHostMalloc(&h_block, tail * 8, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(OXH_ERR_NOMEM, "chunk overlap: pinned result");
        }
        oxh::poison_device(d_block, (n * (1 + (own_lens ? 1 : 0) + words) + tail) * 8, st), oxh::poison_pinned(h_block, tail * 8);
        d_first = d_block;
        d_lens = own_lens ? d_first + n : nullptr;
        d_member = (unsigned long long*)(d_first + n * (own_lens ? 2 : 1));
        d_matrix = d_member + n * words;
        d_sets = (uint64_t*)(d_matrix + 2 * cells + 1);
        memcpy(h_block + 2 * cells + 1, set_first, (nsets + 1) * 8);
        return OXH_OK;
    }

    // mark and count over first[] on `st`, then the matrices to the caller; complete on return
    int run(const uint64_t* lens_on_device, uint64_t* rows_out, uint64_t* bytes_out, hipStream_t st) {
        HIP_TRY(hipMemsetAsync(d_member, 0, (n * words + 2 * cells + 1) * 8, st));
        HIP_TRY(hipMemcpyAsync(d_sets, h_block + 2 * cells + 1, (nsets + 1) * 8, hipMemcpyHostToDevice, st));
        // at most 2 048 workgroups have rows (as the resolve's grid), each `chunk` contiguous rows of one set
        const uint64_t chunk = std::max<uint64_t>(256, ((n + 2047) / 2048 + 255) / 256 * 256);
        uint64_t longest = 1;
        for (uint64_t k = 0; k < nsets; ++k) longest = std::max(longest, h_block[2 * cells + 2 + k] - h_block[2 * cells + 1 + k]);
        const dim3 grid((unsigned)((longest + chunk - 1) / chunk), (unsigned)nsets);
        oxh::overlap_mark_kernel<<<grid, 256, 0, st>>>(d_first, d_sets, (uint32_t)words, n, chunk, d_member, d_matrix + 2 * cells);
        HIP_TRY(hipGetLastError());
        oxh::overlap_count_kernel<<<grid, 256, 0, st>>>(d_first, bytes_out ? lens_on_device : nullptr, d_sets, (uint32_t)nsets,
                                                       (uint32_t)words, n, chunk, d_member, d_matrix, d_matrix + 2 * cells);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_block, d_matrix, (2 * cells + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (const uint64_t e = h_block[2 * cells]) {
            std::string m = "oxh_chunk_overlap: ";
            if (e & oxh::kErrFirst) m += "a first ordinal is not below the row count; ";
            if (e & oxh::kErrSetBit) m += "a membership word holds a bit of no set; ";
            return fail(OXH_ERR_HIP, m + "no result");
        }
        memcpy(rows_out, h_block, cells * 8);
        if (bytes_out) memcpy(bytes_out, h_block + cells, cells * 8);
        return OXH_OK;
    }

    void release(hipStream_t st, bool failed) {
        if (failed && ix) (void)hipStreamSynchronize(st);  // work of a failed call may still be queued
        if (d_block) (void)hipFree(d_block);
        if (h_block) (void)hipHostFree(h_block);
        if (ix) (void)oxh_dedup_index_destroy(ix);
    }
};

int overlap_enter(oxh_ctx* ctx, const uint64_t* set_first, uint64_t nsets, uint64_t* rows_out, uint64_t* bytes_out, bool& done) {
    done = false;
    int rc = check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    if (set_first[nsets] == 0) {
        memset(rows_out, 0, nsets * nsets * 8);
        if (bytes_out) memset(bytes_out, 0, nsets * nsets * 8);
        done = true;
        return OXH_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

}  // namespace

extern "C" {

int oxh_dedup_index_create(oxh_ctx* ctx, uint64_t capacity_rows, void** out) {
    if (!out) return fail(OXH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int rc = check_device(ctx ? ctx->device : 0);  // OXH_ERR_NODEVICE before anything else: there is no CPU index
    if (rc) return rc;
    if (!ctx) return fail(OXH_ERR_INVALID, "ctx is NULL");
    if (capacity_rows > kMaxRows) return fail(OXH_ERR_INVALID, "capacity_rows above 2^40");
    HIP_TRY(hipSetDevice(ctx->device));
    DedupIndex* ix = new DedupIndex();
    ix->ctx = ctx;
    ix->device = ctx->device;
    ix->key_cap = capacity_rows ? capacity_rows : kDefaultRows;
    ix->slots = pow2_at_least(2 * ix->key_cap);
    auto cleanup = [&](int code, const char* m) {
        oxh_dedup_index_destroy(ix);
        (void)hipGetLastError();
        return fail(code, m);
    };
    if (hipMalloc(&ix->d_keys, ix->key_cap * 16) != hipSuccess) return cleanup(OXH_ERR_NOMEM, "dedup index: key store");
    if (hipMalloc(&ix->d_table, ix->slots * 8) != hipSuccess) return cleanup(OXH_ERR_NOMEM, "dedup index: table");
    if (hipMalloc(&ix->d_ctrl, 8 * sizeof(unsigned long long)) != hipSuccess) return cleanup(OXH_ERR_NOMEM, "dedup index: control words");
    if (hipHostMalloc(&ix->h_ctrl, 8 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return cleanup(OXH_ERR_NOMEM, "dedup index: pinned control words");
    oxh::poison_device(ix->d_keys, ix->key_cap * 16, ctx->stream), oxh::poison_device(ix->d_table, ix->slots * 8, ctx->stream);
    oxh::poison_device(ix->d_ctrl, 8 * sizeof(unsigned long long), ctx->stream), oxh::poison_pinned(ix->h_ctrl, 8 * sizeof(unsigned long long));
    if (hipMemsetAsync(ix->d_table, 0xFF, ix->slots * 8, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return cleanup(OXH_ERR_HIP, "dedup index: clearing the table");
    *out = ix;
    return OXH_OK;
}

int oxh_dedup_index_destroy(void* index) {
    if (!index) return OXH_OK;
    DedupIndex* ix = as_index(index);
    if (!ix) return fail(OXH_ERR_INVALID, "not a dedup index");
    (void)hipSetDevice(ix->device);
    if (ix->d_keys) (void)hipFree(ix->d_keys);
    if (ix->d_table) (void)hipFree(ix->d_table);
    if (ix->d_ctrl) (void)hipFree(ix->d_ctrl);
    if (ix->h_ctrl) (void)hipHostFree(ix->h_ctrl);
    if (ix->d_piece) (void)hipFree(ix->d_piece);
    if (ix->h_piece) (void)hipHostFree(ix->h_piece);
    ix->magic = 0;
    delete ix;
    return OXH_OK;
}

int oxh_dedup_index_insert_device(void* index, const uint64_t* d_digests, const uint64_t* d_lens, uint64_t n, uint64_t* d_first,
                                  uint64_t* stats, void* stream) {
    DedupIndex* ix = as_index(index);
    if (!ix) return fail(OXH_ERR_INVALID, "not a dedup index");
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return OXH_OK;
    if (!d_digests) return fail(OXH_ERR_INVALID, "d_digests is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    int rc = enter(ix);
    if (rc) return rc;
    return insert_rows(ix, d_digests, hipMemcpyDeviceToDevice, d_lens, n, n, d_first, stats, (hipStream_t)stream);
}

int oxh_dedup_index_insert_host(void* index, const uint64_t* digests, const uint64_t* lens, uint64_t n, uint64_t* first,
                                uint64_t* stats) {
    DedupIndex* ix = as_index(index);
    if (!ix) return fail(OXH_ERR_INVALID, "not a dedup index");
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return OXH_OK;
    if (!digests) return fail(OXH_ERR_INVALID, "digests is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    int rc = enter(ix);
    if (rc || (rc = piece_buffers(ix))) return rc;
    hipStream_t st = ix->ctx->stream;
    uint64_t *h_dig = ix->h_piece, *h_len = h_dig + 2 * kPieceRows, *h_first = h_len + kPieceRows;
    uint64_t *d_len = ix->d_piece + 2 * kPieceRows, *d_first = d_len + kPieceRows;
    // a later row never lowers an earlier row's answer (its ordinal is larger), so pieces in order give
    // what one insert of all n rows gives
    for (uint64_t at = 0; at < n; at += kPieceRows) {
        const uint64_t m = std::min(kPieceRows, n - at);
        memcpy(h_dig, digests + 2 * at, m * 16);
        if (lens) {
            memcpy(h_len, lens + at, m * 8);
            HIP_TRY(hipMemcpyAsync(d_len, h_len, m * 8, hipMemcpyHostToDevice, st));
        }
        rc = insert_rows(ix, h_dig, hipMemcpyHostToDevice, lens ? d_len : nullptr, m, n - at, first ? d_first : nullptr, stats, st);
        if (rc) return rc;
        if (first) {
            HIP_TRY(hipMemcpyAsync(h_first, d_first, m * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            memcpy(first + at, h_first, m * 8);
        }
    }
    return OXH_OK;
}

int oxh_dedup_index_query_device(void* index, const uint64_t* d_digests, uint64_t n, uint64_t* d_first, void* stream) {
    DedupIndex* ix = as_index(index);
    if (!ix) return fail(OXH_ERR_INVALID, "not a dedup index");
    if (n == 0) return OXH_OK;
    if (!d_digests || !d_first) return fail(OXH_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    int rc = enter(ix);
    if (rc) return rc;
    return query_rows(ix, d_digests, n, d_first, (hipStream_t)stream);
}

int oxh_dedup_index_query_host(void* index, const uint64_t* digests, uint64_t n, uint64_t* first) {
    DedupIndex* ix = as_index(index);
    if (!ix) return fail(OXH_ERR_INVALID, "not a dedup index");
    if (n == 0) return OXH_OK;
    if (!digests || !first) return fail(OXH_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    int rc = enter(ix);
    if (rc || (rc = piece_buffers(ix))) return rc;
    hipStream_t st = ix->ctx->stream;
    uint64_t *h_dig = ix->h_piece, *h_first = h_dig + 3 * kPieceRows;
    uint64_t *d_dig = ix->d_piece, *d_first = d_dig + 3 * kPieceRows;
    for (uint64_t at = 0; at < n; at += kPieceRows) {
        const uint64_t m = std::min(kPieceRows, n - at);
        memcpy(h_dig, digests + 2 * at, m * 16);
        HIP_TRY(hipMemcpyAsync(d_dig, h_dig, m * 16, hipMemcpyHostToDevice, st));
        if ((rc = query_rows(ix, d_dig, m, d_first, st))) return rc;
        HIP_TRY(hipMemcpyAsync(h_first, d_first, m * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(first + at, h_first, m * 8);
    }
    return OXH_OK;
}

int oxh_dedup_index_counts(void* index, uint64_t* out4) {
    DedupIndex* ix = as_index(index);
    if (!ix) return fail(OXH_ERR_INVALID, "not a dedup index");
    if (!out4) return fail(OXH_ERR_INVALID, "out4 is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    for (int k = 0; k < 4; ++k) out4[k] = ix->life[k];
    return OXH_OK;
}

int oxh_chunk_overlap_device(oxh_ctx* ctx, const uint64_t* d_digests, const uint64_t* d_lens, const uint64_t* set_first,
                             uint64_t nsets, uint64_t* rows_out, uint64_t* bytes_out, void* stream) {
    int rc = overlap_arguments(d_digests, d_lens, set_first, nsets, rows_out, bytes_out);
    if (rc) return rc;
    bool done = false;
    if ((rc = overlap_enter(ctx, set_first, nsets, rows_out, bytes_out, done)) || done) return rc;
    hipStream_t st = (hipStream_t)stream;
    Overlap ov;
    rc = ov.make(ctx, set_first, nsets, false, st);
    if (rc == OXH_OK) rc = insert_rows(ov.ix, d_digests, hipMemcpyDeviceToDevice, nullptr, ov.n, ov.n, ov.d_first, nullptr, st);
    if (rc == OXH_OK) rc = ov.run(d_lens, rows_out, bytes_out, st);
    ov.release(st, rc != OXH_OK);
    return rc;
}

int oxh_chunk_overlap_host(oxh_ctx* ctx, const uint64_t* digests, const uint64_t* lens, const uint64_t* set_first,
                           uint64_t nsets, uint64_t* rows_out, uint64_t* bytes_out) {
    int rc = overlap_arguments(digests, lens, set_first, nsets, rows_out, bytes_out);
    if (rc) return rc;
    bool done = false;
    if ((rc = overlap_enter(ctx, set_first, nsets, rows_out, bytes_out, done)) || done) return rc;
    hipStream_t st = ctx->stream;
    const bool with_lens = lens && bytes_out;
    Overlap ov;
    rc = ov.make(ctx, set_first, nsets, with_lens, st);
    if (rc == OXH_OK) rc = piece_buffers(ov.ix);
    if (rc == OXH_OK)
        rc = [&]() -> int {
            uint64_t *h_dig = ov.ix->h_piece, *h_len = h_dig + 2 * kPieceRows;
            // pieces in order give the first[] of one insert of all the rows (oxh_dedup_index_insert_host);
            // the first piece makes room for the whole call, which the index already has
            for (uint64_t at = 0; at < ov.n; at += kPieceRows) {
                const uint64_t m = std::min(kPieceRows, ov.n - at);
                memcpy(h_dig, digests + 2 * at, m * 16);
                if (with_lens) {
                    memcpy(h_len, lens + at, m * 8);
                    HIP_TRY(hipMemcpyAsync(ov.d_lens + at, h_len, m * 8, hipMemcpyHostToDevice, st));
                }
                int r = insert_rows(ov.ix, h_dig, hipMemcpyHostToDevice, nullptr, m, ov.n - at, ov.d_first + at, nullptr, st);
                if (r) return r;  // complete on return: the pinned piece is free again
            }
            return ov.run(ov.d_lens, rows_out, bytes_out, st);
        }();
    ov.release(st, rc != OXH_OK);
    return rc;
}

}  // extern "C"
