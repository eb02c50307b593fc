"""Writes tests/golden/parquet/lists_*.parquet, the list fixtures of the Parquet reader, with pyarrow (run once, by
hand; the tests need no pyarrow). One table -- tests/_parquet_lists_cases.py's cells(ROWS): five list columns beside
two flat ones -- in row groups of 500 rows and pages of about 100 level entries:
  lists_v1         DataPage V1 without a page index (pages need not begin with a row), uncompressed, dictionaries
                   limited to 1 500 bytes: chunks start dictionary-coded and fall back to PLAIN
  lists_v2         DataPage V2, uncompressed, the same dictionaries
  lists_v1_snappy  lists_v1 with SNAPPY pages
  lists_v2_zstd    lists_v2 with ZSTD pages
lists_split_rows is written by hand (write_split_rows: pyarrow begins every page with a row, this file's pages do not),
and nested_struct / list_of_strings, 10 rows each: a struct column (refused at open) and a list<string> column beside
an int64 one (opens; the list is marked unreadable)."""
import os
import sys

import pyarrow as pa
import pyarrow.parquet as pq

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _parquet_lists_cases as K  # noqa: E402

ARROW = {"<i8": pa.int64(), "<i4": pa.int32(), "<f4": pa.float32(), "<f8": pa.float64()}


class Thrift:
    """The compact protocol, as far as a footer and a page header need it."""

    def __init__(self):
        self.out, self.last = bytearray(), [0]

    def varint(self, v):
        while v >= 0x80:
            self.out.append(v & 0x7F | 0x80)
            v >>= 7
        self.out.append(v)

    def field(self, fid, kind):
        self.out.append((fid - self.last[-1]) << 4 | kind)   # the ids rise by less than 16
        self.last[-1] = fid

    def i32(self, fid, v, kind=5):
        self.field(fid, kind)
        self.varint(v << 1)   # zigzag of a value that is not negative

    def i64(self, fid, v):
        self.i32(fid, v, 6)

    def binary(self, fid, b):
        self.field(fid, 8)
        self.string(b)

    def string(self, b):
        self.varint(len(b))
        self.out += b

    def list(self, fid, elem, n):
        self.field(fid, 9)
        self.out.append(n << 4 | elem)   # fewer than 15 elements

    def begin(self, fid=None):
        if fid is not None:
            self.field(fid, 12)
        self.last.append(0)

    def end(self):
        self.out.append(0)
        self.last.pop()


def packed_run(levels, width):
    """One bit-packed run of the RLE / bit-packed hybrid over all the levels (groups of 8, zeros behind the last)."""
    groups = (len(levels) + 7) // 8
    bits = sum(v << (k * width) for k, v in enumerate(levels))
    t = Thrift()
    t.varint(groups << 1 | 1)
    return bytes(t.out) + bits.to_bytes(groups * width, "little")


def write_split_rows(path):
    """A list<int64> column (optional list, optional elements) in uncompressed V1 pages of K.SPLIT_PAGE level entries,
    cut wherever a row is: what a V1 writer without a page index may do and pyarrow's does not."""
    cells = K.split_cells(K.SPLIT_ROWS)
    entries = []   # (repetition level, definition level, value)
    for cell in cells:
        if not cell:
            entries.append((0, 0 if cell is None else 1, None))
        for j, e in enumerate(cell or []):
            entries.append((1 if j else 0, 2 if e is None else 3, e))
    body = bytearray(b"PAR1")
    for at in range(0, len(entries), K.SPLIT_PAGE):
        page = entries[at:at + K.SPLIT_PAGE]
        rep, deff = packed_run([r for r, _, _ in page], 1), packed_run([d for _, d, _ in page], 2)
        data = len(rep).to_bytes(4, "little") + rep + len(deff).to_bytes(4, "little") + deff + b"".join(v.to_bytes(8, "little") for _, d, v in page if d == 3)
        t = Thrift()
        t.i32(1, 0), t.i32(2, len(data)), t.i32(3, len(data))
        t.begin(5), t.i32(1, len(page)), t.i32(2, 0), t.i32(3, 3), t.i32(4, 3), t.end()
        t.out.append(0)
        body += t.out + data
    t = Thrift()
    t.i32(1, 1)
    t.list(2, 12, 4)
    t.begin(), t.binary(4, b"schema"), t.i32(5, 1), t.end()
    t.begin(), t.i32(3, 1), t.binary(4, b"v"), t.i32(5, 1), t.i32(6, 3), t.end()
    t.begin(), t.i32(3, 2), t.binary(4, b"list"), t.i32(5, 1), t.end()
    t.begin(), t.i32(1, 2), t.i32(3, 1), t.binary(4, b"element"), t.end()
    t.i64(3, len(cells))
    t.list(4, 12, 1)
    t.begin()
    t.list(1, 12, 1)
    t.begin(), t.i64(2, 4), t.begin(3)
    t.i32(1, 2), t.list(2, 5, 2), t.varint(0), t.varint(3 << 1), t.list(3, 8, 3), t.string(b"v"), t.string(b"list"), t.string(b"element")
    t.i32(4, 0), t.i64(5, len(entries)), t.i64(6, len(body) - 4), t.i64(7, len(body) - 4), t.i64(9, 4)
    t.end(), t.end()
    t.i64(2, len(body) - 4), t.i64(3, len(cells))
    t.end()
    t.out.append(0)
    with open(path, "wb") as f:
        f.write(bytes(body) + bytes(t.out) + len(t.out).to_bytes(4, "little") + b"PAR1")
    assert pq.read_table(path).column("v").to_pylist() == cells   # pyarrow reads the hand-cut pages as the cells
    print(path, os.path.getsize(path), "pages", -(-len(entries) // K.SPLIT_PAGE))


def main():
    cells = K.cells(K.ROWS)
    fields = []
    for name, dtype, list_null, element_null, size in K.LISTS:
        element = pa.field("element", ARROW[dtype], nullable=element_null)
        fields.append(pa.field(name, pa.list_(element, size) if size else pa.list_(element), nullable=list_null))
    fields += [pa.field("i", pa.int64()), pa.field("s", pa.string())]
    table = pa.table([pa.array(cells[f.name], f.type) for f in fields], schema=pa.schema(fields))
    out = os.path.join(HERE, "parquet")
    common = dict(row_group_size=500, data_page_size=600, write_batch_size=100, write_statistics=False, use_dictionary=True, dictionary_pagesize_limit=1500)
    variants = {"lists_v1": dict(data_page_version="1.0", write_page_index=False, compression="none"),
                "lists_v2": dict(data_page_version="2.0", compression="none"),
                "lists_v1_snappy": dict(data_page_version="1.0", write_page_index=False, compression="snappy"),
                "lists_v2_zstd": dict(data_page_version="2.0", compression="zstd")}
    for name, how in variants.items():
        path = os.path.join(out, name + ".parquet")
        pq.write_table(table, path, **common, **how)
        print(path, os.path.getsize(path))
    small = dict(compression="none", write_statistics=False)
    pq.write_table(pa.table({"a": pa.array(range(10), pa.int64()), "st": pa.array([{"x": r, "y": float(r)} for r in range(10)])}),
                   os.path.join(out, "nested_struct.parquet"), **small)
    pq.write_table(pa.table({"a": pa.array(range(10), pa.int64()), "ls": pa.array([["t%d" % r] * (r % 3) for r in range(10)], pa.list_(pa.string()))}),
                   os.path.join(out, "list_of_strings.parquet"), **small)
    write_split_rows(os.path.join(out, "lists_split_rows.parquet"))


if __name__ == "__main__":
    main()
