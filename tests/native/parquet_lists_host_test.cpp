// tests/native/parquet_lists_host_test.cpp -- what parquet_read_host.hpp plans for list columns, on the CPU: which
// schemas are a three-level LIST (whatever the middle group and the element are called) and their levels, which are
// still refused at open, the relaxed num_values check, the page list of a list column from hand-made page records,
// the row count per row group, and oxh_parquet_lists_*'s argument checks. With a file's path as its argument it
// walks that (uncompressed) file's page headers instead and prints how many data pages of its list columns begin
// with a repetition level that is not 0, i.e. in the middle of a row. Also what a sanitizer build runs.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "../../oxen_amd/csrc/parquet_host.hpp"
#include "../../oxen_amd/csrc/parquet_read_host.hpp"

namespace pq = oxh::parquet;
namespace pr = oxh::pqr;

struct El {
    const char* name;
    int type, repetition, children, list;  // type -1: a group; list 1: converted type LIST, 2: logical type LIST
};

// A footer of one row group of `rows` rows over `els` (the root first), chunk c holding num_values[c].
static pr::Footer footer_of(const std::vector<El>& els, int64_t rows, const std::vector<int64_t>& num_values) {
    pq::Thrift t;
    t.i32(1, 1);
    t.list(2, pq::kTStruct, els.size());
    for (const El& e : els) {
        t.begin();
        if (e.type >= 0) t.i32(1, e.type);
        if (&e != &els[0]) t.i32(3, e.repetition);
        t.binary(4, e.name, strlen(e.name));
        if (e.type < 0) t.i32(5, e.children);
        if (e.list == 1) t.i32(6, 3);
        if (e.list == 2) t.begin(10), t.begin(3), t.end(), t.end();
        t.end();
    }
    t.i64(3, rows);
    t.list(4, pq::kTStruct, 1);
    t.begin();
    t.list(1, pq::kTStruct, num_values.size());
    for (size_t c = 0; c < num_values.size(); ++c) {
        t.begin(), t.i64(2, 0), t.begin(3);
        t.i32(1, 2), t.i32(4, 0), t.i64(5, num_values[c]), t.i64(6, 100), t.i64(7, 100), t.i64(9, 4 + 100 * (int64_t)c);
        t.end(), t.end();
    }
    t.i64(2, 100 * (int64_t)num_values.size()), t.i64(3, rows);
    t.end();
    t.out.push_back(0);
    const uint64_t at = 4 + 100 * num_values.size();
    return pr::read_footer(t.out.data(), t.out.size(), at, at + t.out.size() + 8);
}

static bool says(const pr::Footer& f, const char* what) { return f.error.find(what) != std::string::npos; }

// The data pages of the file's list columns that begin in the middle of a row; -1: not a file this walk reads.
static long pages_that_continue_a_row(const std::vector<uint8_t>& file) {
    uint64_t at = 0, len = 0;
    if (file.size() < 12 || !pr::footer_place(file.data(), file.data() + file.size() - 8, file.size(), at, len).empty()) return -1;
    const pr::Footer f = pr::read_footer(file.data() + at, len, at, file.size());
    if (!f.error.empty()) return -1;
    long found = 0;
    for (size_t k = 0; k < f.chunks.size(); ++k) {
        if (!f.leaves[k % f.leaves.size()].list) continue;
        const pr::Chunk& c = f.chunks[k];
        uint64_t pos = 0, seen = 0;
        while (pos < c.bytes && seen < c.num_values) {
            pr::Span s{file.data() + c.at + pos, c.bytes - pos, 0, false};
            pr::PageInfo h;
            uint64_t st[pr::kSkipDepth];
            if (!pr::page_header(s, h, st) || h.csize < 0 || (uint64_t)h.csize > s.n - s.at) return -1;
            const uint8_t* body = s.p + s.at;
            if (h.type == pr::kPageData || h.type == pr::kPageDataV2) {
                const bool v1 = h.type == pr::kPageData;
                if (v1 && h.csize < 4) return -1;
                pr::Span rep{body + (v1 ? 4 : 0), v1 ? pr::le32(body) : (uint64_t)h.rep_len, 0, false};
                if (rep.n > (uint64_t)h.csize - (v1 ? 4 : 0)) return -1;
                pr::Run r;
                if (!pr::next_run(rep, 1, (uint64_t)h.num_values, r)) return -1;
                found += (r.packed ? pr::extract(r.body, r.avail, 0, 1) : r.value) != 0;
                seen += (uint64_t)h.num_values;
            }
            pos += s.at + (uint64_t)h.csize;
        }
    }
    return found;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        std::vector<uint8_t> file;
        FILE* in = fopen(argv[1], "rb");
        if (!in) return 2;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof buf, in)) > 0;) file.insert(file.end(), buf, buf + n);
        fclose(in);
        printf("%ld\n", pages_that_continue_a_row(file));
        return 0;
    }
    const El root3{"schema", -1, 0, 2, 0}, flat{"a", pr::kInt64, 1, 0, 0};
    // the three-level LIST under every spelling, with max definition level 3, 1 and 2
    {
        const pr::Footer f = footer_of({root3, flat, {"v", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"element", pr::kInt64, 1, 0, 0}}, 10, {10, 25});
        assert(f.error.empty() && f.leaves.size() == 2 && !f.leaves[0].list && f.chunks[1].num_values == 25);
        const pr::Leaf& v = f.leaves[1];
        assert(v.list && v.name == "v" && v.physical == pr::kInt64 && !v.required && v.cause.empty());
        assert(v.def_list == 1 && v.def_slot == 2 && v.max_def == 3 && pr::level_width(v.max_def) == 2);
        assert(pr::native_type(v.physical) == OXH_CSV_INT64);
    }
    {
        const pr::Footer f = footer_of({root3, {"e", -1, 0, 1, 2}, {"bag", -1, 2, 1, 0}, {"array_element", pr::kFloat, 0, 0, 0}, flat}, 10, {80, 10});
        assert(f.error.empty() && f.leaves.size() == 2 && f.leaves[0].list && f.leaves[0].required && !f.leaves[1].list);
        assert(f.leaves[0].def_list == 0 && f.leaves[0].def_slot == 1 && f.leaves[0].max_def == 1 && pr::level_width(1) == 1);
    }
    {
        const pr::Footer f = footer_of({{"schema", -1, 0, 1, 0}, {"t", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"item", pr::kInt32, 0, 0, 0}}, 10, {10});
        assert(f.error.empty() && f.leaves[0].list && f.leaves[0].def_list == 1 && f.leaves[0].def_slot == 2 && f.leaves[0].max_def == 2 && pr::level_width(2) == 2);
    }
    // a list of strings opens and is the column's own refusal
    {
        const pr::Footer f = footer_of({root3, flat, {"ls", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"element", pr::kByteArray, 1, 0, 0}}, 10, {10, 12});
        assert(f.error.empty() && f.leaves[1].list && f.leaves[1].cause == "a list of BYTE_ARRAY is not read" && f.leaves[0].cause.empty());
    }
    // still refused at open, with the messages of a file without lists: a struct, a list of lists, a list of structs,
    // the legacy repeated leaf; and the root's count
    assert(says(footer_of({root3, flat, {"st", -1, 1, 2, 0}, {"x", pr::kInt64, 1, 0, 0}, {"y", pr::kDouble, 1, 0, 0}}, 10, {10, 10, 10}), "column 'st' is a nested field (a group of 2)"));
    assert(says(footer_of({root3, flat, {"ll", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"element", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"element", pr::kInt64, 1, 0, 0}}, 10, {10, 10}),
                "column 'll' is a nested field"));
    assert(says(footer_of({root3, flat, {"ls", -1, 1, 1, 1}, {"list", -1, 2, 2, 0}, {"x", pr::kInt64, 1, 0, 0}, {"y", pr::kInt64, 1, 0, 0}}, 10, {10, 10, 10}), "column 'ls' is a nested field"));
    assert(says(footer_of({root3, flat, {"r", pr::kInt64, 2, 0, 0}}, 10, {10, 14}), "column 'r' is a repeated field (repetition levels are not read)"));
    assert(says(footer_of({{"schema", -1, 0, 3, 0}, flat, {"v", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"element", pr::kInt64, 1, 0, 0}}, 10, {10, 10}), "the schema's root names 3 children, the schema has 2"));
    // num_values: a list's chunk counts level entries, a row has one at least
    const std::vector<El> one_list{root3, flat, {"v", -1, 1, 1, 1}, {"list", -1, 2, 1, 0}, {"element", pr::kInt64, 1, 0, 0}};
    assert(footer_of(one_list, 10, {10, 10}).error.empty());
    assert(says(footer_of(one_list, 10, {10, 9}), "column 'v': num_values 9 is less than the group's 10 rows"));
    assert(says(footer_of(one_list, 10, {11, 25}), "column 'a': num_values 11 is not the group's 10 rows"));
    // the page list: a dictionary page, a V1 page (the walk leaves the repetition stream where a flat page has its
    // definition levels), a V2 page; the second chunk's first page is marked again
    {
        pr::Footer f = footer_of(one_list, 10, {10, 200});
        f.group_rows = {6, 4}, f.chunks.resize(4);
        std::vector<pr::ChunkDesc> chunks(4);
        chunks[1].page0 = 0, chunks[3].page0 = 3;
        const std::vector<uint32_t> counts{0, 3, 0, 1};
        std::vector<pr::PageRec> recs(4);
        recs[0] = pr::PageRec{1000, 80, (uint32_t)pr::kPageDict, 10, (uint32_t)pr::kEncPlain, 0, 0, 0, 0, 80, 0};
        recs[1] = pr::PageRec{1100, 300, (uint32_t)pr::kPageData, 130, (uint32_t)pr::kEncRleDict, 4, 17, 21, pr::kPageInImage, 120, 0};
        recs[2] = pr::PageRec{1500, 400, (uint32_t)pr::kPageDataV2, 40, (uint32_t)pr::kEncPlain, 9, 11, 20, 1, 400, 0};
        recs[3] = pr::PageRec{2000, 400, (uint32_t)pr::kPageDataV2, 30, (uint32_t)pr::kEncPlain, 2, 3, 5, 1, 400, 0};
        const pr::ColumnPages cp = pr::list_pages(f, 1, chunks, counts, recs);
        assert(cp.cause.empty() && cp.data.empty() && cp.lists.size() == 3 && cp.dicts.size() == 1 && cp.entries == 10 && cp.indices && cp.words == 3 + 1 + 1);
        const pr::ListPage &a = cp.lists[0], &b = cp.lists[1], &c = cp.lists[2];
        assert(a.rep_at == 4 && a.rep_bytes == 17 && a.def_at == ~0u && a.values_at == 21 && a.dict == 0 && a.in_image == 1 && a.first == 1 && a.group == 0 && a.word0 == 0);
        assert(b.rep_at == 0 && b.rep_bytes == 9 && b.def_at == 9 && b.def_bytes == 11 && b.values_at == 20 && b.dict == ~0u && b.first == 0 && b.word0 == 3);
        assert(c.first == 1 && c.group == 1 && c.word0 == 4 && c.num_values == 30);
        const uint32_t good[3] = {4, 2, 4}, moved[3] = {5, 2, 3};
        assert(pr::list_rows_error(f, cp, good).empty());
        assert(pr::list_rows_error(f, cp, moved) == "row group 0: its pages start 7 rows, the group has 6");
        recs[2].flags |= 2;
        assert(pr::list_pages(f, 1, chunks, counts, recs).cause == "row group 0, page 2: levels that are not RLE");
        recs[2].flags = 1, recs[2].encoding = 5;
        assert(pr::list_pages(f, 1, chunks, counts, recs).cause.find("value encoding 5 is not read") != std::string::npos);
        recs[2].encoding = (uint32_t)pr::kEncPlain, recs[1].values_at = 301;
        assert(pr::list_pages(f, 1, chunks, counts, recs).cause.find("its levels do not fit its 300 bytes") != std::string::npos);
    }
    // the type words and the entry's argument checks
    {
        assert(pr::is_list_word(OXH_PARQUET_LIST | OXH_CSV_FLOAT32) && pr::is_list_word(OXH_PARQUET_LIST | OXH_PARQUET_LIST64 | OXH_CSV_INT64));
        assert(!pr::is_list_word(OXH_CSV_INT64) && !pr::is_list_word(OXH_PARQUET_LIST64 | OXH_CSV_INT64) && !pr::is_list_word(OXH_PARQUET_LIST | 1024));
        assert(pr::element_word(OXH_PARQUET_LIST | OXH_PARQUET_LIST64 | OXH_CSV_INT32) == OXH_CSV_INT32 && pr::list_cell_bytes(OXH_PARQUET_LIST | OXH_CSV_INT32) == 4);
        const uint32_t col[1] = {1}, type[1] = {OXH_PARQUET_LIST | OXH_PARQUET_LIST64 | OXH_CSV_INT64}, flat_type[1] = {OXH_CSV_INT64};
        uint64_t bytes[1], stats[4], capacity[1] = {80};
        alignas(8) uint8_t block[96];
        void* values[1] = {block};
        void* offsets[1] = {block + 4};
        uint8_t* bitmap[1] = {block};
        pr::ListsArgs a{10, 2, 1, col, type, capacity, nullptr, nullptr, nullptr, nullptr, bytes, stats};
        assert(pr::lists_error(a).empty());  // the measure
        a.types = flat_type;
        assert(pr::lists_error(a).find("which is not OXH_PARQUET_LIST on a fixed-width element's word") != std::string::npos);
        a.types = type, a.values = values;
        assert(pr::lists_error(a) == "only some of values, offsets, validity and child_validity are NULL");
        a.offsets = offsets, a.validity = bitmap, a.child_validity = bitmap;
        assert(pr::lists_error(a) == "selection 0: offsets is not aligned to its entries");
        offsets[0] = block + 8;
        assert(pr::lists_error(a).empty());
    }
    printf("ok\n");
    return 0;
}
