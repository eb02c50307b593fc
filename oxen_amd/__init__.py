"""oxen_amd -- MI355X-native content-hashing stage for Oxen's `oxen add` / commit indexing path.

XXH3-128 (the digest liboxen stores for every file, util/hasher.rs) computed by hand-written
gfx950 HIP kernels behind the C ABI in include/oxen_hash.h (oxen_amd/liboxen_hash.so).

Modules:
  hasher    -- mirror of liboxen `util::hasher` (same names / errors) plus batched forms
  merkle    -- MerkleHash and the commit-time parent-node streams (K2)
  version_store -- verify-before-publish writes (AtomicFile.with_hash, LocalVersionStore)
  dedup     -- fixed-size and FastCDC chunking + chunk digests (block-level dedup), and the
               device-resident dedup index that says which chunks are duplicates (DedupIndex);
               chunk overlap between the versions of a file (chunk_overlap, OxenChunker)
  tabular   -- row hashes of a data frame from its columns and the row set-diff (`oxen diff` on
               tabular files: df_hash_rows, df_hash_rows_on_cols, compute_new_row_indices), and the
               keyed diff of two frames (keyed_diff_digests, diff_dfs) with its contents: the take of
               the joined rows' columns on the device (take, diff_contents, diff_dfs_contents), and the
               stable multi-column row sort (sort_indices, sort_by; `sort=True` of the contents), and the
               rows grouped by equality on key columns (group_rows, unique, unique_count, is_duplicated,
               n_duped_rows), and the rows a `--filter` selects (parse_filter, filter_terms, filter_rows, filter_df),
               and the embedding query: mean of the selected vectors, cosine similarity of every row, the ranked
               page (embedding_mean, cosine_similarity, embedding_take, nearest_neighbors, sort_by_similarity),
               and the CSV file itself: read on the device (read_csv, read_csv_device) and written there (write_csv,
               write_csv_device, write_df), and the same columns as JSON Lines or one JSON array (write_jsonl, write_json and their
               _device forms), and JSON Lines read on the device (read_jsonl, read_jsonl_device, read_df)
  procpool  -- file hashing sharded over reader processes (the open/close floor is per process)
  shard     -- multi-GPU sharding and the RCCL digest gather
  device    -- device-resident (HBM) batch entry points over torch buffers
  workloads -- deterministic synthetic inputs for the BASELINE.json configs
  build     -- hipcc build of the in-tree library
"""
from ._capi import OxenError  # noqa: F401

__version__ = "0.1.0"

# re-exported from oxen_amd.dedup on first use (that module imports torch; `import oxen_amd` does not)
_FROM_DEDUP = ("ChunkOverlap", "chunk_overlap", "chunk_overlap_device", "names_to_digests", "count_commit_overlap",
               "OxenChunker")
# and from oxen_amd.tabular
_FROM_TABULAR = ("KeyedDiff", "STATUS_NAMES", "keyed_diff_digests", "keyed_diff_digests_device", "diff_dfs",
                 "take", "take_device", "diff_contents", "diff_dfs_contents", "output_columns", "columns_to_arrow",
                 "sort_indices", "sort_indices_device", "sort_orders_from_arrow", "sort_by", "sort_diff_rows_device",
                 "RowGroups", "GroupStats", "group_rows", "group_rows_device", "unique", "unique_count", "is_duplicated",
                 "n_duped_rows", "FilterExpr", "FilterStats", "RowFilter", "parse_filter", "filter_terms", "filter_rows",
                 "filter_rows_device", "filter_df", "Embedding", "EmbeddingStats", "Similarity", "embedding", "embedding_from_arrow",
                 "embedding_to_arrow", "embedding_mean", "embedding_mean_device", "cosine_similarity", "cosine_similarity_device",
                 "embedding_take", "embedding_take_device", "page_rows", "nearest_neighbors", "nearest_neighbors_device",
                 "sort_by_similarity", "sort_by_similarity_device", "concat", "concat_device", "slice_range", "parse_slice",
                 "slice_rows", "slice_rows_device", "head", "head_device", "tail", "tail_device", "page", "page_device", "vstack",
                 "vstack_device", "CsvStats", "CsvColumnStats", "CsvFile", "CSV_TYPE_NAMES", "read_csv", "read_csv_device", "csv_shape",
                 "csv_schema", "CsvWriteStats", "write_csv", "write_csv_device", "write_df", "JsonWriteStats", "write_jsonl",
                 "write_jsonl_device", "write_json", "write_json_device", "JsonlStats", "JsonlFile", "read_jsonl", "read_jsonl_device",
                 "jsonl_shape", "jsonl_schema", "read_df")


def __getattr__(name):
    if name in _FROM_DEDUP:
        from . import dedup

        return getattr(dedup, name)
    if name in _FROM_TABULAR:
        from . import tabular

        return getattr(tabular, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
