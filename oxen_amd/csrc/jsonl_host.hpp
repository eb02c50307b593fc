// oxen_amd/csrc/jsonl_host.hpp -- the host-only pieces of oxh_jsonl_* (jsonl_read.hip): what oxh_jsonl_open_*
// checks before it needs a device, in the header's order; the size of every working array of the index; the
// class-bits-to-type rule of the inference; and the names from the key text that comes down. The column entries
// share their checks, sizes and the deferred floats' conversion with the CSV reader (csv_host.hpp). Plain C++ with
// no HIP in it, so that a stand-alone program can call it (tests/native/jsonl_host_test.cpp, which is also what a
// sanitizer build runs).
#pragma once

#include <string>
#include <unordered_map>
#include <vector>

#include "csv_host.hpp"
#include "jsonl_text.hpp"

namespace oxh::jsonl {

constexpr uint64_t kMaxNames = 65535;
constexpr uint32_t kCarryChunk = 8;  // tiles one lane of a carry kernel folds one after the other

// "" when oxh_jsonl_open_*'s arguments are well formed, else what is wrong with them, in the header's order.
inline std::string open_error(const uint8_t* bytes, uint64_t nbytes, uint64_t infer_rows, uint32_t flags, void* const* out,
                              const uint64_t* stats8) {
    if (infer_rows == 0) return "infer_rows is 0 (UINT64_MAX means every row)";
    if (flags) return "unknown flags";
    if (nbytes >= csv::kMaxBytes) return "a buffer of 2^32 bytes and more (positions are u32)";
    if (nbytes && !bytes) return "bytes is NULL";
    if (!out) return "out is NULL";
    if (!stats8) return "stats8 is NULL";
    return "";
}

// The inference's rule over the AND of a column's class bits: a column with no cell but nulls is a string column.
inline uint32_t type_of_bits(uint32_t bits, bool all_null) { return csv::type_of_bits(bits, all_null); }

// open, first lease: per 4 KiB tile the backslash carry and the carry into it, the line carry (flags, d0, d1) and
// the state it is entered with (parity, depth), the kept and record-end counts and their scans -- 56 B per tile
// -- and the two scans' tile sums.
struct IndexLease {
    uint64_t ctrl, esc, esc_in, flags, d0, d1, par_in, depth_in, kept, kept_scan, recs, rec_scan, kept_sums, rec_sums, total;
    explicit IndexLease(uint64_t tiles) {
        csv::Carver carve;
        ctrl = carve(csv::kCtrlBytes);
        esc = carve(tiles * 4), esc_in = carve(tiles * 4);
        flags = carve(tiles * 4), d0 = carve(tiles * 4), d1 = carve(tiles * 4);
        par_in = carve(tiles * 4), depth_in = carve(tiles * 8);
        kept = carve(tiles * 4), kept_scan = carve(tiles * 8);
        recs = carve(tiles * 4), rec_scan = carve(tiles * 8);
        const uint64_t sums = (csv::scan_tiles_of(tiles) + 1) * 8;
        kept_sums = carve(sums), rec_sums = carve(sums);
        total = carve.at;
    }
};

// open, the schema's lease: per 64 rows of the window the listed rows' mask word, their count and its scan; per
// listed row its key count and key bytes and their scans (24 B per row of the window).
struct SchemaLease {
    uint64_t ctrl, mask, counts, bases, list, nkeys, key_bytes, nkeys_scan, bytes_scan, sums, total;
    explicit SchemaLease(uint64_t window) {
        const uint64_t blocks = csv::blocks_of(window);
        csv::Carver carve;
        ctrl = carve(csv::kCtrlBytes);
        mask = carve(blocks * 8), counts = carve(blocks * 4), bases = carve(blocks * 8);
        list = carve(window * 4), nkeys = carve(window * 4), key_bytes = carve(window * 4);
        nkeys_scan = carve(window * 8), bytes_scan = carve(window * 8);
        sums = carve((csv::scan_tiles_of(std::max(window, blocks)) + 1) * 8);
        total = carve.at;
    }
};

// The names of the schema: the unescaped keys in order of first appearance.
struct Names {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets{0};
    std::unordered_map<std::string, uint32_t> index;
    uint64_t count() const { return offsets.size() - 1; }
    // One key as its string token; true: it was new.
    bool add_token(const uint8_t* tok, uint32_t n) {
        std::string name(n, '\0');
        const uint32_t len = unescape_copy(tok, n, (uint8_t*)name.data(), n);
        name.resize(std::min<uint32_t>(len, n));
        if (!index.emplace(name, (uint32_t)count()).second) return false;
        bytes.insert(bytes.end(), name.begin(), name.end());
        offsets.push_back(bytes.size());
        return true;
    }
    // The keys of the listed rows as they come down: key_lens[k] bytes each, one after the other in text.
    void add_keys(const uint32_t* key_lens, uint64_t nkeys, const uint8_t* text) {
        uint64_t at = 0;
        for (uint64_t k = 0; k < nkeys; ++k) {
            add_token(text + at, key_lens[k]);
            at += key_lens[k];
        }
    }
};

}  // namespace oxh::jsonl
