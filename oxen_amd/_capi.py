"""ctypes binding of the C ABI in include/oxen_hash.h (oxen_amd/liboxen_hash.so).

Loading never falls back to anything: if the library is missing the import of a hashing entry
point raises, and on a host without a gfx950 device `Context()` raises `OxenError`.
"""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboxen_hash.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "oxen_hash.h")

OXH_OK = 0
OXH_ERR_INVALID = 1
OXH_ERR_HIP = 2
OXH_ERR_IO = 3
OXH_ERR_NOMEM = 4
OXH_ERR_NODEVICE = 5
OXH_ERR_META = 6
OXH_ERR_OPEN = 7
OXH_META_NONE = 0
OXH_META_GIVEN = 1
OXH_META_TEXT = 2
OXH_META_ERROR = 3
OXH_MODE_AUTO = 0
OXH_MODE_WAVE = 1
OXH_MODE_LANE = 2
OXH_MODE_WAVE_SHORT = 3
OXH_MODE_WAVE_PACKED = 4
OXH_MAX_STAGING_BYTES = 2147483392  # 2 GiB - 256 (include/oxen_hash.h)
OXH_COMM_ID_BYTES = 128
OXH_COL_FIXED1 = 1    # Int8
OXH_COL_FIXED4 = 4    # Int32, Float32
OXH_COL_FIXED8 = 8    # Int64, Float64, Datetime(ms)
OXH_COL_BOOL = 16     # Arrow bit-packed booleans
OXH_COL_BYTES32 = 32  # bytes + int32 offsets
OXH_COL_BYTES64 = 64  # bytes + int64 offsets
OXH_KEYED_DIFF_KEEP_UNCHANGED = 1
OXH_KEYED_DIFF_NONE = 0xFFFFFFFF
OXH_DIFF_UNCHANGED = 0
OXH_DIFF_ADDED = 1
OXH_DIFF_REMOVED = 2
OXH_DIFF_MODIFIED = 3
OXH_TAKE_NULL = 0xFFFFFFFF        # an absent index (the value of OXH_KEYED_DIFF_NONE)
OXH_TAKE_NO_COLUMN = 0xFFFFFFFF   # no fallback source column
OXH_CONCAT_MAX_PARTS = 65536      # the most parts of one oxh_concat_columns_* call
OXH_SORT_SIGNED = 0     # two's complement of the column's width
OXH_SORT_UNSIGNED = 1   # plain unsigned of the column's width
OXH_SORT_FLOAT = 2      # numeric; -0.0 == +0.0; every NaN equal and above +inf (widths 4 and 8)
OXH_FILTER_EQ = 0       # the operators of a filter term, `column OP literal`
OXH_FILTER_NE = 1
OXH_FILTER_LT = 2
OXH_FILTER_LE = 3
OXH_FILTER_GT = 4
OXH_FILTER_GE = 5
OXH_FILTER_AND = 0      # the logical operators between terms, folded left to right
OXH_FILTER_OR = 1
OXH_FILTER_MAX_TERMS = 16
OXH_FILTER_MAX_LITERAL_BYTES = 4096   # all byte literals of one call together
OXH_EMB_FIXED = 0       # the layouts of an embedding column: Arrow FixedSizeList<float32>[dim]
OXH_EMB_LIST32 = 1      # Arrow List<float32>: int32 offsets in elements
OXH_EMB_LIST64 = 2      # Arrow LargeList<float32>: int64 offsets in elements
OXH_CSV_NO_QUOTE = 256  # no byte is a quote
OXH_CSV_HAS_HEADER = 1  # flags: the first kept record names the columns
OXH_CSV_INT64 = 1       # the types of a CSV column
OXH_CSV_FLOAT64 = 2
OXH_CSV_BOOL = 3
OXH_CSV_STRING = 4      # OXH_COL_BYTES32
OXH_CSV_STRING64 = 5    # OXH_COL_BYTES64
OXH_JSON_LINES = 0      # flags of oxh_write_json_*: one object per row and line
OXH_JSON_ARRAY = 1      # one array of the rows' objects

_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32
_u64p = ctypes.POINTER(ctypes.c_uint64)
_i32p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p
_int = ctypes.c_int

# name -> (restype, argtypes); must mirror include/oxen_hash.h exactly (tests/test_capi.py checks).
SIGNATURES = {
    "oxh_abi_version": (_int, []),
    "oxh_last_error": (ctypes.c_char_p, []),
    "oxh_device_count": (_int, [ctypes.POINTER(_int)]),
    "oxh_ctx_create": (_int, [_int, _u64, ctypes.POINTER(_vp)]),
    "oxh_ctx_destroy": (_int, [_vp]),
    "oxh_ctx_stream": (_vp, [_vp]),
    "oxh_xxh3_128_batch_device": (_int, [_vp, _vp, _vp, _u64, _vp, _int, _vp]),
    "oxh_chunk_digests_device": (_int, [_vp, _u64, _u64, _vp, _vp]),
    "oxh_xxh3_128_large_device": (_int, [_vp, _vp, _u64, _vp, _vp]),
    "oxh_xxh3_128_large_batch_device": (_int, [ctypes.POINTER(_vp), _u64p, _u64, _vp, _vp]),
    "oxh_hash_buffers": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u64p]),
    "oxh_hash_files": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, _u64p, _u64p, _i32p]),
    "oxh_hash_files_meta": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u64p, _u64p, _i32p]),
    "oxh_hash_files_ex": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u64p, _u64p, _i32p, _i32p, _u64p,
                                 _i32p]),
    "oxh_add_files": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, ctypes.c_char_p, _u64p, _u64p, _i32p, _i32p]),
    "oxh_add_files_ex": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, ctypes.c_char_p, _u64p, _u64p, _i32p, _i32p,
                                _i32p]),
    "oxh_clean_corrupted_versions": (_int, [_vp, ctypes.c_char_p, _int, _u64p]),
    "oxh_hash_files_text": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, _u64p, _u64p, _i32p, _u64p]),
    "oxh_xxh3_128_text_batch_device": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "oxh_hash_files_text_utf8": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, _u64p, _u64p, _i32p, _u64p, _i32p]),
    "oxh_files_modified": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64p, _vp, _u64p, _vp, _vp, _vp, _vp,
                                  _u64, _vp, _i32p, _u64p]),
    "oxh_files_modified_ex": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64p, _vp, _u64p, _vp, _vp, _vp, _vp,
                                     _u64, _vp, _i32p, _i32p, _u64p]),
    "oxh_pool_create": (_int, [_vp, _int, _int, _int, _u64, ctypes.POINTER(_vp)]),
    "oxh_pool_hash_files": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _vp, _u64, _u64p, _u64p, _i32p]),
    "oxh_pool_hash_files_ex": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _vp, _u64, _u64p, _u64p, _i32p, _i32p]),
    "oxh_pool_size": (_int, [_vp, ctypes.POINTER(_int), _vp]),
    "oxh_pool_destroy": (_int, [_vp]),
    "oxh_utf8_prefix_device": (_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "oxh_combined_hash_device": (_int, [_vp, _vp, _u64, _vp, _vp]),
    "oxh_hash_streams": (_int, [_vp, _vp, _u64p, _u64p, _u64, _u64p]),
    "oxh_format_hex": (_int, [_u64, _u64, ctypes.c_char_p]),
    "oxh_format_dec": (_int, [_u64, _u64, ctypes.c_char_p]),
    "oxh_fill_splitmix": (_int, [_vp, _u64, _u64, _vp]),
    "oxh_set_kernel_variant": (_int, [_int]),
    "oxh_set_scratch_poison": (_int, [_int]),
    "oxh_scratch_poisoned_bytes": (_u64, []),
    "oxh_xxh3_stream_create": (_int, [_vp, ctypes.POINTER(_vp)]),
    "oxh_xxh3_stream_update": (_int, [_vp, _vp, _u64]),
    "oxh_xxh3_stream_digest": (_int, [_vp, _u64p]),
    "oxh_xxh3_stream_reset": (_int, [_vp]),
    "oxh_xxh3_stream_destroy": (_int, [_vp]),
    "oxh_fastcdc_device": (_int, [_vp, _u64p, _u64p, _u64, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u64, _u64p, _vp]),
    "oxh_fastcdc_max_chunks": (_u64, [_u64p, _u64, _u32]),
    "oxh_fastcdc_files": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, _u32, _u32, _u32, _u32, _u64p, _u64p, _u64p,
                                 _u64, _u64p, _u64p, _i32p, _i32p]),
    "oxh_fastcdc_host": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u32, _u32, _u32, _u32, _u64p, _u64p,
                                _u64p, _u64, _u64p]),
    "oxh_chunk_digests_files": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64, _u64, _u64p, _u64, _u64p, _u64p, _i32p,
                                       _i32p]),
    "oxh_chunk_digests_host": (_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u64, _u64p, _u64, _u64p]),
    "oxh_fastcdc_files_multi": (_int, [ctypes.POINTER(_vp), _int, ctypes.POINTER(ctypes.c_char_p), _u64, _u32, _u32, _u32,
                                       _u32, _u64p, _u64p, _u64p, _u64, _u64p, _u64p, _i32p, _i32p]),
    "oxh_chunk_digests_files_multi": (_int, [ctypes.POINTER(_vp), _int, ctypes.POINTER(ctypes.c_char_p), _u64, _u64, _u64p,
                                             _u64, _u64p, _u64p, _i32p, _i32p]),
    "oxh_fastcdc_host_multi": (_int, [ctypes.POINTER(_vp), _int, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u32, _u32,
                                      _u32, _u32, _u64p, _u64p, _u64p, _u64, _u64p]),
    "oxh_chunk_digests_host_multi": (_int, [ctypes.POINTER(_vp), _int, ctypes.POINTER(ctypes.c_char_p), _u64p, _u64, _u64,
                                            _u64p, _u64, _u64p]),
    "oxh_fastcdc_gear": (_int, [_u64p]),
    "oxh_fastcdc_masks": (_int, [_u32, _u32, _u64p, _u64p]),
    "oxh_dedup_index_create": (_int, [_vp, _u64, ctypes.POINTER(_vp)]),
    "oxh_dedup_index_destroy": (_int, [_vp]),
    "oxh_dedup_index_insert_device": (_int, [_vp, _vp, _vp, _u64, _vp, _u64p, _vp]),
    "oxh_dedup_index_insert_host": (_int, [_vp, _u64p, _u64p, _u64, _u64p, _u64p]),
    "oxh_dedup_index_query_device": (_int, [_vp, _vp, _u64, _vp, _vp]),
    "oxh_dedup_index_query_host": (_int, [_vp, _u64p, _u64, _u64p]),
    "oxh_dedup_index_counts": (_int, [_vp, _u64p]),
    "oxh_chunk_overlap_device": (_int, [_vp, _vp, _vp, _u64p, _u64, _u64p, _u64p, _vp]),
    "oxh_chunk_overlap_host": (_int, [_vp, _u64p, _u64p, _u64p, _u64, _u64p, _u64p]),
    "oxh_row_hashes_device": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                     ctypes.POINTER(_vp), _u64p, _vp, _vp]),
    "oxh_row_hashes_host": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                   ctypes.POINTER(_vp), _u64p, _u64p]),
    "oxh_row_diff_device": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64p, _vp]),
    "oxh_row_diff_host": (_int, [_vp, _u64p, _u64, _u64p, _u64, ctypes.POINTER(_u32), ctypes.POINTER(_u32), _u64p]),
    "oxh_keyed_diff_device": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64p, _u32, _u64, _vp, _vp, _vp, _u64p,
                                     _vp]),
    "oxh_keyed_diff_host": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64p, _u32, _u64, _vp, _vp, _vp, _u64p]),
    "oxh_take_columns_device": (_int, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                       ctypes.POINTER(_vp), _u64p, _u64p, _u64, _vp, _vp, _u32, ctypes.POINTER(_u32), _u64p,
                                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p,
                                       ctypes.POINTER(_u32), _vp]),
    "oxh_take_columns_host": (_int, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                     ctypes.POINTER(_vp), _u64p, _u64p, _u64, _vp, _vp, _u32, ctypes.POINTER(_u32), _u64p,
                                     ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p,
                                     ctypes.POINTER(_u32)]),
    "oxh_concat_columns_device": (_int, [_vp, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                         ctypes.POINTER(_vp), _u64p, _u64p, _u64p, _u64p, _u64p, ctypes.POINTER(_vp),
                                         ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _vp]),
    "oxh_concat_columns_host": (_int, [_vp, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                       ctypes.POINTER(_vp), _u64p, _u64p, _u64p, _u64p, _u64p, ctypes.POINTER(_vp),
                                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32)]),
    "oxh_sort_rows_device": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                    ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _vp, _u64p, _vp]),
    "oxh_sort_rows_host": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                  ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _vp, _u64p]),
    "oxh_group_rows_device": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                     ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _vp, _vp, _vp, _vp, _u64p, _vp]),
    "oxh_group_rows_host": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                   ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _vp, _vp, _vp, _vp, _u64p]),
    "oxh_filter_rows_device": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                      ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _u32, ctypes.POINTER(_u32),
                                      ctypes.POINTER(_u32), _u64p, _vp, _u64p, ctypes.POINTER(_u32), _vp, _vp, _u64p, _vp]),
    "oxh_filter_rows_host": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                    ctypes.POINTER(_vp), _u64p, ctypes.POINTER(_u32), _u32, ctypes.POINTER(_u32),
                                    ctypes.POINTER(_u32), _u64p, _vp, _u64p, ctypes.POINTER(_u32), _vp, _vp, _u64p]),
    "oxh_embedding_mean_device": (_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64p, _vp]),
    "oxh_embedding_mean_host": (_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64p]),
    "oxh_embedding_similarity_device": (_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64p, _vp]),
    "oxh_embedding_similarity_host": (_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64p]),
    "oxh_embedding_take_device": (_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64p, _vp]),
    "oxh_embedding_take_host": (_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64p]),
    "oxh_csv_open_device": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, ctypes.POINTER(_vp), _u64p, _vp]),
    "oxh_csv_open_host": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, ctypes.POINTER(_vp), _u64p]),
    "oxh_csv_close": (_int, [_vp]),
    "oxh_csv_header": (_int, [_vp, _vp, _u64, _u64p, _u64p]),
    "oxh_csv_infer": (_int, [_vp, _u64, ctypes.POINTER(_u32)]),
    "oxh_csv_columns_device": (_int, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), _u64p, ctypes.POINTER(_vp),
                                      ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _u64p, _vp]),
    "oxh_csv_columns_host": (_int, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), _u64p, ctypes.POINTER(_vp),
                                    ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _u64p]),
    "oxh_write_csv_device": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_vp),
                                    ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _vp, _u64p, _u32, _u32, _u32, _vp, _u64,
                                    _u64p, _u64p, _vp]),
    "oxh_write_csv_host": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_vp),
                                  ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _vp, _u64p, _u32, _u32, _u32, _vp, _u64,
                                  _u64p, _u64p]),
    "oxh_write_json_device": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_vp),
                                     ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _vp, _u64p, _u32, _vp, _u64, _u64p, _u64p,
                                     _vp]),
    "oxh_write_json_host": (_int, [_vp, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_vp),
                                   ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _vp, _u64p, _u32, _vp, _u64, _u64p, _u64p]),
    "oxh_jsonl_open_device": (_int, [_vp, _vp, _u64, _u64, _u32, ctypes.POINTER(_vp), _u64p, _vp]),
    "oxh_jsonl_open_host": (_int, [_vp, _vp, _u64, _u64, _u32, ctypes.POINTER(_vp), _u64p]),
    "oxh_jsonl_close": (_int, [_vp]),
    "oxh_jsonl_names": (_int, [_vp, _vp, _u64, _u64p, _u64p]),
    "oxh_jsonl_infer": (_int, [_vp, ctypes.POINTER(_u32)]),
    "oxh_jsonl_columns_device": (_int, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), _u64p, ctypes.POINTER(_vp),
                                        ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _u64p, _vp]),
    "oxh_jsonl_columns_host": (_int, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), _u64p, ctypes.POINTER(_vp),
                                      ctypes.POINTER(_vp), ctypes.POINTER(_vp), _u64p, _u64p]),
    "oxh_comm_check": (_int, [_int]),
    "oxh_ctx_counters": (_int, [_vp, _u64p, _int]),
    "oxh_comm_unique_id": (_int, [ctypes.c_char_p]),
    "oxh_comm_create": (_int, [ctypes.c_char_p, _int, _int, _int, ctypes.POINTER(_vp)]),
    "oxh_comm_info": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "oxh_gather_digests": (_int, [_vp, _vp, _u64p, _vp, _int, _vp]),
    "oxh_comm_destroy": (_int, [_vp]),
}

_lib = None


class OxenError(Exception):
    """Mirror of liboxen's OxenError for this path (error/mod.rs); carries the C status code."""

    def __init__(self, msg: str, code: int = OXH_ERR_INVALID):
        super().__init__(msg)
        self.code = code


def header_symbols() -> list[str]:
    """Every function the public header declares."""
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:[\w\*\s]+?)\b(oxh_\w+)\s*\(", text, flags=re.M)))


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OxenError(f"{LIB_PATH} is missing: run `python -m oxen_amd.build` (no CPU fallback exists)",
                            OXH_ERR_NODEVICE)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != OXH_OK:
        msg = lib().oxh_last_error().decode(errors="replace")
        raise OxenError(f"{what} failed (status {rc}): {msg}", rc)


def device_count() -> int:
    n = _int(0)
    check(lib().oxh_device_count(ctypes.byref(n)), "oxh_device_count")
    return n.value


class Context:
    """An oxh_ctx: streams + pinned staging on one device."""

    def __init__(self, device: int = 0, staging_bytes: int = 0):
        h = _vp()
        check(lib().oxh_ctx_create(int(device), int(staging_bytes), ctypes.byref(h)), "oxh_ctx_create")
        self.handle = h
        self.device = device

    @property
    def stream(self) -> int:
        return lib().oxh_ctx_stream(self.handle) or 0

    def counters(self) -> dict:
        """oxh_ctx_counters: large-file piece-buffer allocations and their current bytes, file requests
        served on the caller's thread, file-engine runs, staged slots submitted, and the most items of
        1 MiB and more one slot held."""
        out = (ctypes.c_uint64 * 6)()
        check(lib().oxh_ctx_counters(self.handle, out, 6), "oxh_ctx_counters")
        return {"big_allocs": int(out[0]), "big_bytes": int(out[1]), "direct_requests": int(out[2]),
                "engine_runs": int(out[3]), "slots": int(out[4]), "slot_large_max": int(out[5])}

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().oxh_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
