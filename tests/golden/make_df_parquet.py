"""Writes tests/golden/parquet/*.parquet, the Parquet reader's fixtures, with pyarrow (run once, by hand; the tests
need no pyarrow). One table -- tests/_parquet_cases.py's cells(ROWS) -- in three encodings, all uncompressed, row
groups of 500 rows, pages cut every 100 rows so that neighbouring pages share validity bytes and words:
  v1_dict_fallback  DataPage V1, dictionaries limited to 1 500 bytes: chunks start dictionary-coded and fall back to PLAIN
  v2_dict_fallback  the same with DataPage V2 (RLE booleans)
  v2_plain          DataPage V2 without dictionaries
and two more files: unsupported (unsupported_cells: a FIXED_LEN_BYTE_ARRAY column between two readable ones, pyarrow's
defaults but no compression) and many_pages (many_cells: 60 000 rows, a V2 page every 100 rows, dictionary-coded)."""
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
    os.makedirs(out, exist_ok=True)
    common = dict(compression="none", row_group_size=500, data_page_size=600, write_batch_size=100, write_statistics=False)
    variants = {"v1_dict_fallback": dict(data_page_version="1.0", use_dictionary=True, dictionary_pagesize_limit=1500),
                "v2_dict_fallback": dict(data_page_version="2.0", use_dictionary=True, dictionary_pagesize_limit=1500),
                "v2_plain": dict(data_page_version="2.0", use_dictionary=False)}
    for name, how in variants.items():
        path = os.path.join(out, name + ".parquet")
        pq.write_table(table, path, **common, **how)
        print(path, os.path.getsize(path))
    odd = K.unsupported_cells(K.UNSUPPORTED_ROWS)
    table = pa.table({"a": pa.array(odd["a"], pa.int64()), "fixed": pa.array(odd["fixed"], pa.binary(4)), "d": pa.array(odd["d"], pa.int32()).cast(pa.date32())})
    pq.write_table(table, os.path.join(out, "unsupported.parquet"), compression="none", write_statistics=False)
    many = K.many_cells(K.MANY_ROWS)
    table = pa.table({name: pa.array(many[name], ARROW[dtype]) for name, dtype, _ in K.MANY_COLUMNS})
    pq.write_table(table, os.path.join(out, "many_pages.parquet"), compression="none", write_statistics=False, data_page_version="2.0", use_dictionary=True,
                   data_page_size=1, write_batch_size=100)
    for name in ("unsupported", "many_pages"):
        print(name, os.path.getsize(os.path.join(out, name + ".parquet")))


if __name__ == "__main__":
    main()
