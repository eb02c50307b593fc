// oxen_amd/csrc/parquet_read_device.hpp -- what the Parquet reader's two device files share (parquet_read.hip: the
// open and the flat columns; parquet_lists.hip: the list columns): the handle, a column as the kernels read it, the
// one way to a page's body, the value of a rank, the ballot store and the launch shapes.
#pragma once

#include <memory>

#include "capi_internal.hpp"
#include "columns.hpp"
#include "parquet_read_host.hpp"

namespace oxh {

namespace pqr {
constexpr unsigned long long kErrLevels = 2, kErrIndex = 4, kErrValues = 8, kErrChain = 16, kErrPlace = 32;
// ctrl words of one selected column
constexpr int kColNulls = 0, kColDictValues = 1, kColBytes = 2, kColErr = 3, kColWords = 8;
}  // namespace pqr

// What the column kernels read of one column.
struct PqColumn {
    const uint8_t* bytes;
    const uint8_t* image;  // the inflated bodies of the compressed pages (NULL: the file has none)
    const pqr::DataPage* pages;
    const pqr::DictPage* dicts;
    uint64_t nrows;
    uint32_t npages, ndicts, optional;
    uint64_t* words;       // optional columns: the page-local validity words
    uint32_t* prefix;      // per word: the page's valid rows in front of it
    uint32_t* page_valid;  // per data page
    uint32_t* idx;         // per row: at row0 + rank, the index (or RLE boolean) of the page's value of that rank
    uint32_t *cell_at, *cell_len;  // PLAIN byte arrays: at row0 + rank, the cell in its page's body
    uint32_t *dict_at, *dict_len;  // per dictionary entry: the cell in its page's body
};

// Where a page's body starts: in the file, or in the image once inflated.
template <class Page>
__device__ __forceinline__ const uint8_t* pq_body(const PqColumn& c, const Page& pg) {
    return (pg.in_image ? c.image : c.bytes) + pg.body;
}
// The same for a place the length pass hands to the copy: the top bit says the image.
constexpr uint64_t kPqInImage = 1ull << 63;
template <class Page>
__device__ __forceinline__ uint64_t pq_place(const Page& pg, uint64_t at) { return (pg.body + at) | (pg.in_image ? kPqInImage : 0); }
__device__ __forceinline__ const uint8_t* pq_at(const PqColumn& c, uint64_t place) {
    return (place & kPqInImage ? c.image : c.bytes) + (place & ~kPqInImage);
}

__device__ __forceinline__ void pq_store_word(uint8_t* bitmap, unsigned long long word, uint64_t row0, uint64_t n, unsigned lane) {
    if (bitmap && lane < 8 && row0 + 8 * lane < n) bitmap[(row0 >> 3) + lane] = (uint8_t)(word >> (8 * lane));
}

// Where the value of rank `rank` of width W of page pg starts, NULL (and *bad) where its bytes are not the page's
// or the dictionary's.
template <uint32_t W>
__device__ __forceinline__ const uint8_t* pq_fixed_source(const PqColumn& c, const pqr::DataPage& pg, uint32_t rank, bool& bad) {
    if (pg.dict != ~0u) {
        const pqr::DictPage& d = c.dicts[pg.dict];
        const uint64_t k = c.idx[pg.row0 + rank];
        if ((k + 1) * W > d.body_size) return bad = true, nullptr;
        return pq_body(c, d) + k * W;
    }
    const uint64_t at = (uint64_t)pg.values_at + (uint64_t)rank * W;
    if (at + W > pg.body_size) return bad = true, nullptr;
    return pq_body(c, pg) + at;
}

// SRC: the bytes of a value in the file; DST: of a cell of the output; a 4 -> 8 store sign-extends an integer and
// widens a float exactly.
template <uint32_t SRC, uint32_t DST, bool FLOAT>
__device__ __forceinline__ uint64_t pq_fixed_load(const uint8_t* src) {
    if (SRC == 8) return ld64u(src);
    if (DST == 4) return ld32u(src);
    if (FLOAT) return (uint64_t)__double_as_longlong((double)__uint_as_float(ld32u(src)));
    return (uint64_t)(int64_t)(int32_t)ld32u(src);
}

// pq_index_kernel and pq_clear_kernel (parquet_read.hip) as another file enqueues them: the indices of every
// dictionary-coded page of `c` into c.idx, read by pq_fixed_source; `n` device words to zero.
int pq_index_enqueue(const PqColumn& c, unsigned long long* d_ctrl, hipStream_t st);
int pq_clear_enqueue(unsigned long long* d_words, uint64_t n, hipStream_t st);

constexpr uint64_t kParquetMagic = 0x4F58485051523031ull;  // "OXHPQR01"

struct ParquetHandle {
    uint64_t magic = kParquetMagic;
    oxh_ctx* ctx = nullptr;
    int device = 0;
    const uint8_t* d_bytes = nullptr;
    uint8_t* owned = nullptr;  // the host form's device copy
    uint8_t* image = nullptr;  // the inflated bodies of every compressed page, until close
    uint64_t image_bytes = 0, pages_inflated = 0;
    uint64_t nbytes = 0;
    pqr::Footer footer;
    std::vector<pqr::ColumnPages> columns;  // per column; `cause` where the reader cannot read it
    std::vector<uint8_t> names;
    std::vector<uint64_t> name_offsets;
    uint64_t data_pages = 0, dict_pages = 0;
    ~ParquetHandle() {
        magic = 0;
        if (owned) (void)hipFree(owned);
        if (image) (void)hipFree(image);
    }
    uint64_t nrows() const { return footer.nrows; }
    uint64_t ncols() const { return footer.leaves.size(); }
};

inline ParquetHandle* pq_handle_of(void* p) {
    ParquetHandle* h = (ParquetHandle*)p;
    return h && h->magic == kParquetMagic ? h : nullptr;
}

inline int pq_device_enter(oxh_ctx* ctx) {
    int rc = capi::check_device(ctx ? ctx->device : 0);  // there is no CPU path
    if (rc) return rc;
    if (!ctx) return capi::fail(OXH_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return OXH_OK;
}

inline unsigned pq_cap_grid(uint64_t groups) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(groups, 1), 2048); }
inline unsigned pq_row_grid(uint64_t n) { return pq_cap_grid((n + 255) / 256); }
// The page kernels, a wave per page: at most 512 waves, the rest by grid stride. A page's work is a serial chase of run
// headers or lengths, and a column of more than 512 pages of the usual MiB is half a GiB: the rounds are not what it
// waits for. (Files cut into many small pages pay for it; not measured.)
inline unsigned pq_wave_grid(uint64_t jobs) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((jobs + 3) / 4, 1), 128); }

}  // namespace oxh
