"""The CSV reader on the GPU (oxh_csv_*, oxen_amd/csrc/csv_read.hip; oxen_amd.tabular): both forms against the
restatement of tests/_csv.py -- a sequential byte-by-byte state machine with int() / float() behind the grammars --
for EXACT equality of the whole outputs: values, offsets, validity bytes with the bits past nrows zero, stats8,
stats4, the header's names and the inferred types, every output buffer followed by sentinels that must survive.
Every column is read twice, as its inferred type and as a string column. The edges (the lane, the
wave-instruction, the tile, the scan's tile, the grid cap, the long-cell threshold) are read from the sources and
the hazards placed at every one of them +- 1. The large cases are built from known cells with numpy and compared
with those cells; the restatement parses only the small adversarial parts."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu

FORMS = ["host", "device"]
HERE = os.path.dirname(os.path.abspath(__file__))


def load_restatement():
    """tests/_csv.py by its path: `import _csv` is the C module behind the standard library's csv."""
    import importlib.util
    import sys

    if "_csv_restatement" not in sys.modules:
        spec = importlib.util.spec_from_file_location("_csv_restatement", os.path.join(HERE, "_csv.py"))
        sys.modules[spec.name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[spec.name])
    return sys.modules["_csv_restatement"]


C = load_restatement()
CSVS = os.path.join(HERE, "golden", "data_test", "csvs")
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("csv_read.hip", "csv_host.hpp", "keyed_diff.hip")}
LANE = 16                                     # bytes of one lane's load
WAVE = 64 * LANE                              # bytes of one wave-instruction
TILE = int(re.search(r"constexpr uint32_t kTileBytes = (\d+);", SOURCES["csv_host.hpp"]).group(1))
LONG = int(re.search(r"constexpr uint32_t kLongCell = (\d+);", SOURCES["csv_host.hpp"]).group(1))
SLOT = int(re.search(r"constexpr uint32_t kDeferSlot = (\d+);", SOURCES["csv_host.hpp"]).group(1))
SCAN_PER = int(re.search(r"constexpr uint32_t kScanPer = (\d+), kScanTile = 256 \* kScanPer;", SOURCES["keyed_diff.hip"]).group(1))
SCAN_TILE = 256 * SCAN_PER
CAP = int(re.search(r"unsigned cap_grid\(uint64_t groups\) \{ return \(unsigned\)std::min<uint64_t>\(std::max<uint64_t>\(groups, 1\), (\d+)\); \}",
                    SOURCES["csv_read.hip"]).group(1))
G = CAP * 256                                 # rows of one round of a lane-per-row kernel
ROUND = CAP * TILE                            # bytes of one round of the index kernels
PAD = 32
SENTINEL = 0xA5
assert TILE == 256 * LANE and "csv_lane_masks(base, t * kCsvTileBytes + 16ull * threadIdx.x" in SOURCES["csv_read.hip"]


# ---------------------------------------------------------------- helpers
def host_buffer(data: bytes, misalign: int) -> np.ndarray:
    big = np.zeros(len(data) + 64, dtype=np.uint8)
    at = (misalign - big.ctypes.data) % 16
    view = big[at:at + len(data)]
    view[:] = np.frombuffer(data, dtype=np.uint8)
    assert len(data) == 0 or view.ctypes.data % 16 == misalign
    return view


def device_buffer(data: bytes, misalign: int):
    import torch

    big = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    at = (misalign - big.data_ptr()) % 16
    view = big[at:at + len(data)]
    if data:
        view.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    torch.cuda.synchronize()
    return view


class Got:
    pass


def offsets_dtype(t):
    return np.int64 if t == C.STRING64 else np.int32


def read(ctx, form, data: bytes, sep=",", quote='"', has_header=True, types=None, cols=None, misalign=0, infer_rows=10000, strings=C.STRING):
    """Open, names, inference, the measure, then the columns into buffers followed by PAD sentinel bytes. Every
    column (or `cols`) as its inferred type (or `types`) and once more as a string column."""
    import torch

    device = form == "device"
    buf = device_buffer(data, misalign) if device else host_buffer(data, misalign)
    got = Got()
    with tabular.CsvFile(buf, sep, quote, has_header, ctx=ctx, device=device, stream=ctx.stream if device else None) as f:
        got.stats8, got.names, got.inferred = tuple(f.stats), f.raw_names, f.infer(infer_rows)
        n = f.stats.rows
        if cols is None:
            cols = list(range(f.stats.ncols))
            types = list(got.inferred if types is None else types)
            cols, types = cols + cols, types + [strings] * len(cols)
        got.cols, got.types = cols, types
        sizes, measured = f.measure(cols, types)
        _, _, col_idx, type_words = f._selection(cols, types)
        held, tables, capacity = [], [[], [], []], np.zeros(max(len(cols), 1), dtype=np.uint64)
        for k, t in enumerate(types):
            want = (sizes[k], (n + 1) * np.dtype(offsets_dtype(t)).itemsize if t in (C.STRING, C.STRING64) else 0, (n + 7) // 8)
            capacity[k] = sizes[k]
            three = []
            for which, size in enumerate(want):
                if device:
                    b = torch.full((size + PAD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
                    tables[which].append(b.data_ptr() if size or which != 1 else None)
                else:
                    b = np.full(size + PAD, SENTINEL, dtype=np.uint8)
                    tables[which].append(b.ctypes.data if size or which != 1 else None)
                three.append((b, size))
            held.append(three)
        if device:
            torch.cuda.synchronize()
        m = max(len(cols), 1)
        arrays = [(ctypes.c_void_p * m)(*tables[w]) for w in range(3)]
        if n and cols:
            wrote_sizes, got.stats4 = f._call(len(cols), col_idx, type_words, capacity, *arrays)
            assert wrote_sizes == sizes and got.stats4 == measured, (wrote_sizes, sizes, got.stats4, measured)
        else:
            got.stats4 = measured
        if device:
            torch.cuda.synchronize()
    got.buffers = []
    for three in held:
        out = []
        for b, size in three:
            raw = b.cpu().numpy() if device else b
            assert (raw[size:] == SENTINEL).all(), "bytes past an output were written"
            out.append(raw[:size].copy())
        got.buffers.append(out)
    got.nrows = n
    return got


def want_buffers(b: C.Buffers):
    return [np.ascontiguousarray(b.values).view(np.uint8), np.zeros(0, np.uint8) if b.offsets is None else b.offsets.view(np.uint8), b.validity]


def same_buffers(got, k, want: C.Buffers, who):
    assert got.stats4[k] == want.stats4, (who, "stats4 of selection", k, got.stats4[k], want.stats4)
    if got.nrows == 0:
        return
    for name, g, w in zip(("values", "offsets", "validity"), got.buffers[k], want_buffers(want)):
        if g.size != w.size or not np.array_equal(g, w):
            at = int(np.nonzero(g[:min(g.size, w.size)] != w[:min(g.size, w.size)])[0][:1].sum()) if g.size and w.size else 0
            raise AssertionError((who, "selection", k, name, "sizes", g.size, w.size, "first difference at byte", at,
                                  g[at:at + 8].tolist(), w[at:at + 8].tolist()))


def check(ctx, form, data: bytes, sep=",", quote='"', has_header=True, who=None, **kw):
    """One file in one form against the restatement; returns (got, parsed)."""
    who = (form, who if who is not None else data[:40])
    p = C.parse(data, ord(sep), C.NO_QUOTE if quote is None else ord(quote), has_header)
    got = read(ctx, form, data, sep, quote, has_header, **kw)
    assert got.stats8 == p.stats8, (who, "stats8", got.stats8, p.stats8)
    assert got.names == p.names, (who, got.names, p.names)
    assert got.inferred == C.infer(p, kw.get("infer_rows", 10000)), (who, got.inferred, C.infer(p))
    for k, (c, t) in enumerate(zip(got.cols, got.types)):
        same_buffers(got, k, C.column(p, c, t), who)
    return got, p


# ---------------------------------------------------------------- small adversarial files
SMALL = {
    "nothing": b"",
    "one byte": b"a",
    "one newline": b"\n",
    "one quote": b'"',
    "15 bytes": b"a,b\n1,2\n3,4\n5,6"[:15],
    "16 bytes": b"a,b\n1,2\n3,4\n5,66",
    "17 bytes": b"a,b\n1,2\n3,4\n5,6\n7",
    "only a header": b"id,name,score\n",
    "only a header, no newline": b"id,name,score",
    "no trailing newline": b"a,b\n1,x\n2,y",
    "crlf": b"a,b\r\n1,x\r\n2,y\r\n",
    "crlf, no trailing newline": b"a,b\r\n1,x\r\n2,y\r",
    "a lone cr record": b"a,b\n1,x\n\r\n2,y\n\n\n3,z\n",
    "cr inside": b"a,b\n1\r,x\ry\r\n",
    "ends inside quotes": b'a,b\n1,"x\n2,y\n',
    "ends inside quotes after a newline": b'a,b\n1,x\n"',
    "short and long": b"a,b,c\n1,2,3\n4\n5,6\n7,8,9,10,11\r\n,,\n12,13,14\n",
    "a long record with cr": b"a\n1,2\r\n3\r\n",
    "null column": b"a,b,c\n1,,x\n2,,y\n3,,z\n",
    "quoted empties": b'a,b,c,d\n"",1,"",""\nx,"",1.5,true\n',
    "quoted cells": b'a,b\n"1","x,y"\n"2","he said ""hi"""\n"3","two\nlines"\n',
    "stray quotes": b'a,b\nx"y,1\n"x"y,2\nx"",3\n',
    "quote runs": b'a\n""""\n""""""\n"a""""b"\n"a"""\n',
    "ints": b"a\n0\n-0\n+7\n9223372036854775807\n-9223372036854775808\n9223372036854775808\n-9223372036854775809\n007\n",
    "ints with junk": b"a\n1\n2\n3x\n 4\n5 \n\n6\n",
    "floats": b"a\n1.5\n-2.\n.5\n1e3\n1E-3\ninf\n-Infinity\nnan\n-NaN\n+nan\n0.1\n1e23\n9007199254740993\n1e400\n-1e-400\n0e999\n1e\n",
    "bools": b"a\ntrue\nFALSE\nTrue\nfalsE\nyes\n\n",
    "mixed types": b"i,f,b,s,e\n1,1.5,true,a,\n2,2,false,b,\n3,,TRUE,3,\n,1e5,,,\n",
    "float wins": b"a,b\n1,true\n2.5,1\n",
    "no header": b"1,x\n2,y\n",
    "header names": b'"a,b","c""d",e\r\n1,2,3\n',
    "duplicate separators": b",,,\n,,,\n",
}
EVERY_TYPE = (C.INT64, C.FLOAT64, C.BOOL)
FORCED = {"ints": EVERY_TYPE, "ints with junk": EVERY_TYPE, "floats": EVERY_TYPE, "bools": EVERY_TYPE, "mixed types": EVERY_TYPE,
          "quoted empties": EVERY_TYPE, "quoted cells": EVERY_TYPE, "short and long": EVERY_TYPE, "stray quotes": EVERY_TYPE}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(SMALL))
def test_small_files(ctx, form, name):
    check(ctx, form, SMALL[name], has_header=name != "no header", who=name)
    # the inference picks String where one cell fits no grammar: the typed parsers see such files under a given type
    for t in FORCED.get(name, ()):
        ncols = C.parse(SMALL[name]).ncols
        check(ctx, form, SMALL[name], types=[t] * ncols, who=(name, "as", C.TYPE_NAMES[t]))


@pytest.mark.parametrize("form", FORMS)
def test_other_dialects(ctx, form):
    check(ctx, form, b"a\tb\n1\t'x\ty'\n2\t\"q\n", sep="\t", quote="'", who="tabs and single quotes")
    check(ctx, form, b'a;b\n"1;2";3\n', sep=";", quote=None, who="no quote")
    check(ctx, form, b"a|b\n1|2\n", sep="|", who="pipes")
    check(ctx, form, b"a,b\n1,2\n3,4\n", has_header=False, who="no header")
    check(ctx, form, b"a,b\n1,x\n2.5,y\nz,w\n", infer_rows=1, who="infer from one row")
    check(ctx, form, b"a,b\n1,x\n2,y\n", strings=C.STRING64, who="int64 offsets")


@pytest.mark.parametrize("form", FORMS)
def test_every_misalignment(ctx, form):
    data = b'id,text,x\n' + b"".join(b'%d,"row ""%d"", with\na newline",%d.5\r\n' % (k, k, k) for k in range(40))
    for misalign in range(16):
        check(ctx, form, data, misalign=misalign, who=("misalign", misalign))
        check(ctx, form, data[:17 + misalign], misalign=misalign, who=("misalign, short", misalign))


def buffer_of(length: int, ending: str) -> bytes:
    """A header and records of 25 bytes cut or stretched to exactly `length` bytes. "newline": the last byte ends
    the last record; "none": the end of the buffer does; "inside quotes": the buffer ends inside a quoted field that
    holds a newline and a separator."""
    body = b"id,text\n" + b"".join(b'%06d,"r %06d, ""x"""\n' % (k, k) for k in range(length // 25 + 2))
    tail = {"newline": b"z\n", "none": b",z", "inside quotes": b'7,"a\n,b'}[ending]
    cut = body[:length - len(tail)]
    cut = cut[:cut.rfind(b"\n") + 1]                      # whole records, then one that fills the rest
    data = cut + b"y" * (length - len(cut) - len(tail)) + tail
    assert len(data) == length
    return data


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ending", ["newline", "none", "inside quotes"])
@pytest.mark.parametrize("length", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_buffers_of_a_tile_and_one_byte_around_it(ctx, form, length, ending):
    """The index walks one position past the last byte, where the last record may end: a buffer of exactly a tile's
    bytes has a last tile that holds that position and no byte, and the lane that holds it reads the last byte from
    the tile before. With a buffer that starts 5 bytes into the aligned space the same happens 5 bytes sooner."""
    got, p = check(ctx, form, buffer_of(length, ending), who=("length", length, ending))
    assert got.stats8[7] == (ending == "inside quotes") and got.stats8[1] > 100
    for misalign in (5, 15):
        check(ctx, form, buffer_of(length, ending), misalign=misalign, who=("length", length, ending, "misaligned by", misalign))
        check(ctx, form, buffer_of(length - misalign, ending), misalign=misalign, who=("length", length - misalign, ending, "misaligned by", misalign))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(os.listdir(CSVS)))
def test_golden_files(ctx, form, name):
    data = open(os.path.join(CSVS, name), "rb").read()
    sep = "\t" if name.endswith(".tsv") or name == "tabs.csv" else ","
    check(ctx, form, data, sep=sep, who=name)


@pytest.mark.parametrize("form", FORMS)
def test_stray_quote_fixture_with_and_without_a_quote(ctx, form):
    data = open(os.path.join(CSVS, "spam_ham_data_w_quote.tsv"), "rb").read()
    assert data.count(b'"') == 9
    got, _ = check(ctx, form, data, sep="\t", quote='"', who="parity")
    assert got.stats8[0] == 100
    got, _ = check(ctx, form, data, sep="\t", quote=None, who="OXH_CSV_NO_QUOTE")
    assert got.stats8[0] == 101


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows", [63, 64, 65, 129])
def test_the_ballot_word(ctx, form, rows):
    rng = np.random.default_rng(rows)
    lines = [b"i,f,b,s"]
    for r in range(rows):
        cells = [b"%d" % rng.integers(-10**6, 10**6), b"%d.25" % rng.integers(0, 999), rng.choice([b"true", b"false"]), b"s%d" % r]
        for c in range(4):
            if rng.random() < 0.3:
                cells[c] = rng.choice([b"", b"?"])
        lines.append(b",".join(bytes(x) for x in cells))
    check(ctx, form, b"\n".join(lines) + b"\n", who=("rows", rows))


# ---------------------------------------------------------------- hazards at the byte edges
def filler(length: int) -> bytes:
    """One well-formed record of exactly `length` >= 4 bytes with two string cells."""
    return b"a" * (length - 3) + b",b\n"


HAZARDS = {   # name -> (record bytes, the byte of it that is put AT the edge)
    "quoted newline and separator": (b'"x,\n,y",z\n', 3),          # the '\n' inside the quotes
    "doubled quote": (b'"p""q",r\n', 3),                           # the second quote of the pair: the pair straddles the edge
    "closing quote, separator, opening quote": (b'"a","b"\n', 4),  # the opening quote: the separator is the last byte before
    "quote last and first": (b'"a""",c\n', 3),                     # quotes on both sides of the edge, the cell ends right after
}


def hazard_file(edge: int, delta: int, spacing: int, row: int):
    """(data, parsed): a header, then every hazard with its marked byte at a multiple of `edge` (+ delta), filler
    records of `row` bytes (the last one before a hazard as long as it takes) in between. The expectation is
    composed: the restatement parses the header and the hazards alone, the filler records are known cells."""
    header = b"s,t\n"
    parts, small, rows_before = [header], [header], []
    at, place = len(header), 0
    fill_row = lambda length: [(b"a" * (length - 3), False), (b"b", False)]   # noqa: E731
    rows = []
    for name, (record, mark) in HAZARDS.items():
        place += spacing
        while (place + delta - mark) - at < 4:
            place += edge
        target = place + delta - mark            # where the hazard record starts
        while target - at >= 2 * row:
            parts.append(filler(row)), rows.append(fill_row(row))
            at += row
        parts.append(filler(target - at)), rows.append(fill_row(target - at))   # as long as it takes: 4 bytes or more
        at = target
        assert at == sum(len(x) for x in parts)
        parts.append(record)
        small.append(record)
        rows_before.append(len(rows))
        rows.append(None)                        # the hazard's own rows go here
        at += len(record)
    data = b"".join(parts)
    p = C.parse(b"".join(small), 0x2C, 0x22, True)
    hazard_rows = iter(p.rows)
    tok, _ = C.tokenize(b"".join(small), 0x2C, 0x22)
    assert len(tok) == 1 + len(HAZARDS) and len(p.rows) == len(HAZARDS)        # each hazard is one record
    rows = [r if r is not None else next(hazard_rows) for r in rows]
    nfill = len(rows) - len(HAZARDS)
    s = p.stats8
    stats = (s[0] + nfill, s[1] + nfill, 2, s[3] + 2 * nfill, 0, s[5], s[6], s[7])
    return data, C.Parsed(stats, p.names, rows, 2)


def check_parsed(ctx, form, data, p, who, **kw):
    got = read(ctx, form, data, **kw)
    assert got.stats8 == p.stats8, (who, got.stats8, p.stats8)
    assert got.names == p.names and got.inferred == [C.STRING, C.STRING], (who, got.names, got.inferred)
    for k, (c, t) in enumerate(zip(got.cols, got.types)):
        same_buffers(got, k, C.column(p, c, t), who)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("edge", [LANE, WAVE, TILE], ids=["lane", "wave-instruction", "tile"])
def test_hazards_at_the_small_edges(ctx, form, edge, delta):
    data, p = hazard_file(edge, delta, spacing=max(edge, 64), row=48)
    check_parsed(ctx, form, data, p, (form, edge, delta))
    # the edges are those of the 16-byte aligned space: in a buffer that starts 5 bytes into it they come 5 bytes sooner
    data, p = hazard_file(edge, delta - 5, spacing=max(edge, 64), row=48)
    check_parsed(ctx, form, data, p, (form, edge, delta, "misaligned by 5"), misalign=5)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_hazards_at_the_scan_tile_and_the_grid_round(ctx, form, delta):
    """SCAN_TILE tiles of the quote-count scan and one round of CAP workgroups are both multiples of 8 MiB here:
    four hazards at the first four of them, between 64 KiB cells that a whole wave copies."""
    edge = SCAN_TILE * TILE
    assert edge % ROUND == 0 or ROUND % edge == 0
    data, p = hazard_file(max(edge, ROUND), delta, spacing=max(edge, ROUND), row=1 << 16)
    assert len(data) > 4 * max(edge, ROUND)
    check_parsed(ctx, form, data, p, (form, "scan tile", delta))


# ---------------------------------------------------------------- long cells
@pytest.mark.parametrize("form", FORMS)
def test_cells_around_the_long_cell_threshold(ctx, form):
    lines = [b"s,t"]
    for inner in (LONG - 1, LONG, LONG + 1, LONG + 63, LONG + 64, LONG + 65, 3 * LONG):
        plain = bytes(97 + k % 26 for k in range(inner))
        lines.append(plain + b",u")                                   # unquoted: raw length = inner
        lines.append(b'"' + plain + b'",q')                           # quoted, nothing doubled
        for at in (0, 1, 62, 63, 64, 65, inner // 2, inner - 3, inner - 2):     # a doubled quote at every place of a 64-byte step
            body = bytearray(plain)
            body[at:at + 2] = b'""'
            lines.append(b'"' + bytes(body) + b'",d')
        body = bytearray(plain)
        body[60:68] = b'""""""""'                                     # a run of eight across a step
        body[130:133] = b'"""'                                        # and an odd run
        lines.append(b'"' + bytes(body) + b'",r')
    check(ctx, form, b"\n".join(lines) + b"\n", who="long cells")


# ---------------------------------------------------------------- many rows, from known cells
@functools.lru_cache(maxsize=None)
def many_rows_case():
    """G + 300 rows (more than one round of every lane-per-row kernel) of Int64, Float64, Boolean and a short string,
    every float a multiple of 2^-10 below 64 (at most 12 significant digits: the exact path by construction)."""
    n = G + 300
    rng = np.random.default_rng(5)
    ints = rng.integers(-2**62, 2**62, size=n)
    floats = rng.integers(-2**16, 2**16, size=n) / 1024.0
    bools = rng.random(n) < 0.5
    tags = rng.integers(0, 1000, size=n)
    null = rng.random((n, 4)) < 0.05
    texts = [["" if gone else text for gone, text in zip(null[:, c].tolist(), column)] for c, column in enumerate((
        [str(v) for v in ints.tolist()], [repr(v) for v in floats.tolist()], ["true" if v else "false" for v in bools.tolist()],
        ["t%d" % v for v in tags.tolist()]))]
    data = ("i,f,b,s\n" + "\n".join(map(",".join, zip(*texts))) + "\n").encode()
    assert all(len(repr(x).replace("-", "").replace(".", "").lstrip("0")) <= 15 for x in floats[:2000].tolist())
    valid = ~null
    strings = [s.encode() for s in texts[3]]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=offsets[1:])
    want = [
        C.Buffers(np.where(valid[:, 0], ints, 0).astype(np.int64).view(np.uint64), None, C.pack(valid[:, 0]), (int(null[:, 0].sum()), 0, 0, 8 * n)),
        C.Buffers(np.where(valid[:, 1], floats, 0.0).view(np.uint64), None, C.pack(valid[:, 1]), (int(null[:, 1].sum()), 0, 0, 8 * n)),
        C.Buffers(C.pack(bools & valid[:, 2]), None, C.pack(valid[:, 2]), (int(null[:, 2].sum()), 0, 0, (n + 7) // 8)),
        C.Buffers(np.frombuffer(b"".join(strings), dtype=np.uint8), offsets.astype(np.int32), C.pack(valid[:, 3]),
                  (int(null[:, 3].sum()), 0, 0, int(offsets[-1]))),
    ]
    return data, n, want


@pytest.mark.parametrize("form", FORMS)
def test_more_rows_than_one_round_and_exact_floats(ctx, form):
    data, n, want = many_rows_case()
    assert n > G and len(data) > ROUND
    got = read(ctx, form, data, cols=[0, 1, 2, 3], types=[C.INT64, C.FLOAT64, C.BOOL, C.STRING])
    assert got.stats8 == (n + 1, n, 4, 4 * (n + 1), 0, 0, 0, 0), got.stats8
    assert got.names == [b"i", b"f", b"b", b"s"] and got.inferred == [C.INT64, C.FLOAT64, C.BOOL, C.STRING]
    assert got.stats4[1][2] == 0                                  # no float was deferred
    for k in range(4):
        same_buffers(got, k, want[k], (form, "many rows"))


@functools.lru_cache(maxsize=None)
def repr_case():
    """64 * SCAN_TILE + 65 doubles of random bits (every exponent, the subnormals) as repr() prints them: more
    deferred-count blocks than one tile of the scan."""
    n = 64 * SCAN_TILE + 65
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    bits[:64] &= np.uint64(0x800FFFFFFFFFFFFF)                    # subnormals
    x = bits.view(np.float64)
    bits = np.where(np.isfinite(x), bits, np.uint64(0x3FF8000000000000))
    x = bits.view(np.float64)
    data = ("x\n" + "\n".join(repr(float(v)) for v in x) + "\n").encode()
    return data, n, bits


@pytest.mark.parametrize("form", FORMS)
def test_repr_doubles_are_deferred_and_still_exact(ctx, form):
    data, n, bits = repr_case()
    got = read(ctx, form, data, cols=[0], types=[C.FLOAT64])
    assert got.stats8[:3] == (n + 1, n, 1) and got.inferred == [C.FLOAT64]
    deferred = got.stats4[0][2]
    assert 0 < deferred < n, deferred
    same_buffers(got, 0, C.Buffers(bits, None, C.pack(np.ones(n, bool)), (0, 0, deferred, 8 * n)), (form, "repr doubles"))


@pytest.mark.parametrize("form", FORMS)
def test_deferred_texts_around_the_slot(ctx, form):
    """Deferred cells whose text is below, at and above the slot that comes down with the list, and far above."""
    cells = [b"0." + b"1234567890" * 30, b"1" + b"0" * 400, b"9007199254740993", b"-1e-320", b"+1.7976931348623157e308"]
    for size in (SLOT - 1, SLOT, SLOT + 1):
        cells.append(b"1." + b"7" * (size - 2))
    check(ctx, form, b"x\n" + b"\n".join(cells) + b"\n", who="deferred texts")


# ---------------------------------------------------------------- poison
MIXED = (b'id,score,ok,name,note\n' + b"".join(b'%d,%d.%d,%s,"n""%d",%s\r\n' % (k, k, k * 7919 % 100000, b"true" if k % 3 else b"no", k, b"x" * (k % 9))
                                              for k in range(300)) + b'301,1e23,false,"' + b"y" * (2 * 512) + b'",\n')


@pytest.mark.parametrize("form", FORMS)
def test_results_do_not_depend_on_the_scratch_contents(ctx, form):
    L = _capi.lib()
    results = []
    for byte in (0x00, 0xFF, 0x5A):
        prev = L.oxh_set_scratch_poison(byte)
        try:
            assert prev == -1
            before = L.oxh_scratch_poisoned_bytes()
            got, _ = check(ctx, form, MIXED, who=("poison", hex(byte)))
            assert L.oxh_scratch_poisoned_bytes() > before
        finally:
            L.oxh_set_scratch_poison(-1)
        results.append(got)
    assert results[0].stats4[1][2] > 0                            # some floats went through the deferral
    for other in results[1:]:
        assert other.stats8 == results[0].stats8 and other.stats4 == results[0].stats4
        for a, b in zip(other.buffers, results[0].buffers):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- the Python layer and the chain
def test_read_csv_and_the_metadata(ctx, tmp_path):
    path = tmp_path / "t.tsv"
    path.write_bytes(b"a\tb\tb\n1\tx\t1.5\n2\t\"y\tz\"\t\n")
    frame = tabular.read_csv(path, ctx=ctx)
    assert list(frame) == ["a", "b", "b_duplicated_0"]
    assert frame["a"].kind == _capi.OXH_COL_FIXED8 and frame["a"].values.tolist() == [1, 2]
    assert frame["b"].values.tobytes() == b"xy\tz" and frame["b"].offsets.tolist() == [0, 1, 4]
    assert frame["b_duplicated_0"].values.tolist() == [1.5, 0.0] and frame["b_duplicated_0"].validity.tolist() == [1]
    assert tabular.csv_shape(path, ctx=ctx) == (3, 2)
    assert tabular.csv_schema(path, ctx=ctx) == [("a", "Int64"), ("b", "String"), ("b_duplicated_0", "Float64")]
    frame = tabular.read_csv(b"1,2\n3,4\n", has_header=False, schema={"column_2": "Float64"}, columns=["column_2"], ctx=ctx)
    assert list(frame) == ["column_2"] and frame["column_2"].values.tolist() == [2.0, 4.0]
    assert tabular.read_csv(b"", ctx=ctx) == {} and tabular.csv_shape(b"", ctx=ctx) == (0, 0)
    with pytest.raises(_capi.OxenError):
        tabular.read_csv(b"a\n1\n", delimiter=",,", ctx=ctx)


def device_columns(p, types):
    import torch

    out = []
    for c, t in enumerate(types):
        b = C.column(p, c, t)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")   # noqa: E731
        if t == C.INT64:
            out.append(Column(_capi.OXH_COL_FIXED8, len(p.rows), up(b.values.view(np.int64)), None, up(b.validity)))
        elif t == C.FLOAT64:
            out.append(Column(_capi.OXH_COL_FIXED8, len(p.rows), up(b.values.view(np.float64)), None, up(b.validity)))
        elif t == C.BOOL:
            out.append(Column(_capi.OXH_COL_BOOL, len(p.rows), up(b.values), None, up(b.validity)))
        else:
            out.append(Column(_capi.OXH_COL_BYTES32, len(p.rows), up(b.values), up(b.offsets), up(b.validity)))
    return out


def chain(frame, ctx):
    """filter -> group -> sort -> take over a frame of device columns; everything that comes out, on the host."""
    names = list(frame)
    cols = list(frame.values())
    terms, logical = tabular.filter_terms(frame, "is_correct == true || difficulty > 1")
    selected = tabular.filter_rows_device(cols, terms, logical, ctx=ctx)
    kept = tabular.take_device(cols, selected.idx, ctx=ctx)
    groups = tabular.group_rows_device([kept[names.index("prompt")]], ctx=ctx)
    perm, _ = tabular.sort_indices_device([kept[names.index("difficulty")], kept[names.index("response_time")]], ctx=ctx)
    final = tabular.take_device(kept, perm, ctx=ctx)
    host = lambda t: None if t is None else t.cpu().numpy().view(np.uint8).tolist()   # noqa: E731
    return ([host(selected.idx), host(groups.group), host(groups.count), host(groups.first_idx), host(perm)] +
            [[c.kind, c.nrows, host(c.values), host(c.offsets), host(c.validity)] for c in final])


def test_the_chain_over_a_fixture(ctx):
    data = open(os.path.join(CSVS, "mixed_data_types.csv"), "rb").read()
    import torch

    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    frame = tabular.read_csv_device(d_bytes, ctx=ctx, stream=ctx.stream)
    p = C.parse(data)
    types = C.infer(p)
    assert [C.TYPE_NAMES[t] for t in types] == ["String", "String", "Boolean", "Float64", "Int64"]
    names = [n.decode() for n in p.names]
    assert list(frame) == names == ["prompt", "response", "is_correct", "response_time", "difficulty"]
    want = chain(dict(zip(names, device_columns(p, types))), ctx)
    got = chain(frame, ctx)
    assert got == want
    assert len(got[0]) > 0 and len(got[4]) == len(got[0])
