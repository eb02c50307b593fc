"""Writes tests/golden/parquet/snappy_*.parquet with pyarrow (run once, by hand; the tests need no pyarrow):
make_df_parquet.py's table -- tests/_parquet_cases.py's cells(ROWS) -- in its three encodings and with its options, but
compression="snappy": every page is compressed, those that grow by it too.
  snappy_v1_dict_fallback  DataPage V1: a page's levels are inside the compressed body
  snappy_v2_dict_fallback  DataPage V2: the levels are stored in front of the compressed values (RLE booleans)
  snappy_v2_plain          DataPage V2 without dictionaries"""
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
    common = dict(compression="snappy", row_group_size=500, data_page_size=600, write_batch_size=100, write_statistics=False)
    variants = {"snappy_v1_dict_fallback": dict(data_page_version="1.0", use_dictionary=True, dictionary_pagesize_limit=1500),
                "snappy_v2_dict_fallback": dict(data_page_version="2.0", use_dictionary=True, dictionary_pagesize_limit=1500),
                "snappy_v2_plain": dict(data_page_version="2.0", use_dictionary=False)}
    for name, how in variants.items():
        path = os.path.join(out, name + ".parquet")
        pq.write_table(table, path, **common, **how)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
