"""Writes tests/golden/parquet/zstd_*.parquet with pyarrow (run once, by hand; the tests need no pyarrow):
make_df_parquet_snappy.py's table, variants and options with compression="zstd", and one file whose columns' chunks
are SNAPPY and ZSTD in turn.
  zstd_v1_dict_fallback  DataPage V1: a page's levels are inside the compressed body
  zstd_v2_dict_fallback  DataPage V2: the levels are stored in front of the compressed values
  zstd_v2_plain          DataPage V2 without dictionaries
  zstd_snappy_mixed      V1 with dictionaries, the columns ZSTD and SNAPPY in turn"""
import os
import sys

import pyarrow as pa
import pyarrow.parquet as pq

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _parquet_cases as K  # noqa: E402

ARROW = {"<i8": pa.int64(), "<i4": pa.int32(), "<f4": pa.float32(), "<f8": pa.float64(), "bool": pa.bool_(), "str": pa.string()}


def main():
    cells = K.cells(K.ROWS)
    fields = [pa.field(name, ARROW[dtype], nullable=not required) for name, dtype, required in K.COLUMNS]
    table = pa.table([pa.array(cells[f.name], f.type) for f in fields], schema=pa.schema(fields))
    out = os.path.join(HERE, "parquet")
    common = dict(row_group_size=500, data_page_size=600, write_batch_size=100, write_statistics=False)
    mixed = {f.name: ("zstd", "snappy")[k % 2] for k, f in enumerate(fields)}
    variants = {"zstd_v1_dict_fallback": dict(compression="zstd", data_page_version="1.0", use_dictionary=True, dictionary_pagesize_limit=1500),
                "zstd_v2_dict_fallback": dict(compression="zstd", data_page_version="2.0", use_dictionary=True, dictionary_pagesize_limit=1500),
                "zstd_v2_plain": dict(compression="zstd", data_page_version="2.0", use_dictionary=False),
                "zstd_snappy_mixed": dict(compression=mixed, data_page_version="1.0", use_dictionary=True, dictionary_pagesize_limit=1500)}
    for name, how in variants.items():
        path = os.path.join(out, name + ".parquet")
        pq.write_table(table, path, **common, **how)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
