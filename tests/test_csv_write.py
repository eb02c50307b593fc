"""The CSV writer on the GPU (oxh_write_csv_*, oxen_amd/csrc/csv_write.hip; oxen_amd.tabular): both forms against the
restatement of tests/_csvwrite.py -- a sequential cell-by-cell writer with repr() behind the float digits -- for
EXACT equality of the whole buffer, out_bytes and stats4, every output followed (and preceded) by sentinel bytes that
must survive. The edges (rows per wave and workgroup, the grid cap, the long-cell threshold, the scan's tile, the LDS
span limit) are read from the sources and the cases placed at every one of them +- 1. The large cases are built
from known cells and compared with their known text; the restatement writes only the small adversarial frames.

Not run at its size: the refusal of a single row whose text is 2^32 bytes or more needs a cell of 4 GiB that one wave
counts 512 bytes a step; the check itself (a u64 sum per row against 2^32 in both length kernels) is read, not run."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_csvwrite_call", os.path.join(HERE, "_csvwrite_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
W = K.W
FORMS = ["host", "device"]
CSVS = os.path.join(HERE, "golden", "data_test", "csvs")
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("csv_write.hip", "csv_text.hpp", "keyed_diff.hip")}
WAVE = 64                                     # rows of one wave: a lane per row
assert "const unsigned lane = threadIdx.x & 63" in SOURCES["csv_write.hip"]
GROUP = int(re.search(r"const uint64_t i = t \* stride \+ \(uint64_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x;", SOURCES["csv_write.hip"]).group(1))
CAP = int(re.search(r"constexpr unsigned kCsvwMaxGroups = (\d+);", SOURCES["csv_write.hip"]).group(1))
SPAN = int(re.search(r"constexpr uint32_t kCsvwSpanLds = (\d+);", SOURCES["csv_write.hip"]).group(1))
LONG = int(re.search(r"constexpr uint32_t kLongCell = (\d+);", SOURCES["csv_text.hpp"]).group(1))
SCAN_PER = int(re.search(r"constexpr uint32_t kScanPer = (\d+), kScanTile = 256 \* kScanPer;", SOURCES["keyed_diff.hip"]).group(1))
SCAN_TILE = 256 * SCAN_PER
G = CAP * GROUP                               # rows of one round of a lane-per-row kernel
assert GROUP == 256 and LONG == 512

EDGE_FLOATS = [0.0, -0.0, K.from_bits(0x7FF8000000000000), K.from_bits(0xFFF8000000000000), K.from_bits(0x7FF80000DEADBEEF),
               K.from_bits(0xFFF0000000000001), float("inf"), float("-inf"), 0.1, 19.0, 1e-5, 1e-6, 1.5e-7, 1.25e-7, 1e-22, 999999999999999.0,
               1e15, 1e16, 1.5e16, 123456789012345680.0, 0.1 + 0.2, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
               -0.1, -1e15, -5e-324, 1e-23, 12.5, 1234567890123456.0, 0.001, 100.0]


# ---------------------------------------------------------------- helpers
def same(got: bytes, want: bytes, who):
    if got != want:
        n = min(len(got), len(want))
        at = next((k for k in range(n) if got[k] != want[k]), n)
        raise AssertionError((who, "sizes", len(got), len(want), "first difference at byte", at, got[max(at - 20, 0):at + 20], want[max(at - 20, 0):at + 20]))


def check(ctx, form, names, types, cells, sep=0x2C, quote=0x22, header=True, misalign=0, cols=None, want=None, who=None):
    """One frame in one form against the restatement (or against `want`, a large case's known text and stats)."""
    cols = cols if cols is not None else [K.host_column(t, c) for t, c in zip(types, cells)]
    got, stats = K.write(ctx, form, cols, types, names, sep, quote, header, misalign)
    text, wstats = want if want is not None else W.write(names, types, cells, sep, quote, header)
    assert stats == wstats, (who, "stats4", stats, wstats)
    same(got, text, who)
    return got, stats


def mixed(n, seed=1):
    """n rows of five columns of every type, with nulls, hazards and deferred floats."""
    rng = np.random.default_rng(seed)
    strings = [b"plain", b"", b"a,b", b'say "hi"', b"two\nlines", b"cr\rhere", b"\xc3\xa9t\xc3\xa9", b'"', b'""', b"x" * 40]
    floats = [0.5, 12.25, 0.1 + 0.2, 1e15, -0.0, float("nan"), float("-inf"), 1e-7, 123.456, 5e-324]
    pick = rng.integers(0, 10, size=(n, 5)).tolist()
    null = (rng.random((n, 5)) < 0.12).tolist()
    ints = rng.integers(-10 ** 12, 10 ** 12, size=n).tolist()
    cells = [[None if null[r][0] else ints[r] if pick[r][0] else -(1 << 63) for r in range(n)],
             [None if null[r][1] else floats[pick[r][1]] for r in range(n)],
             [None if null[r][2] else pick[r][2] < 5 for r in range(n)],
             [None if null[r][3] else strings[pick[r][3]] for r in range(n)],
             [None if null[r][4] else strings[pick[r][4]] * (1 + pick[r][0] % 3) for r in range(n)]]
    return [b"i", b"f", b"b", b"s", b"big"], [W.INT64, W.FLOAT64, W.BOOL, W.STRING, W.STRING64], cells


def cells_of(c: Column, t) -> list:
    """A Column of either form as plain cells; a float as its bits (a NaN has no == )."""
    host = lambda x: None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))  # noqa: E731
    n = c.nrows
    validity, values, offsets = host(c.validity), host(c.values), host(c.offsets)
    present = np.ones(n, dtype=bool) if validity is None else np.unpackbits(validity, bitorder="little")[c.validity_bit:c.validity_bit + n].astype(bool)
    if t == W.INT64:
        out = values.view(np.int64).tolist()
    elif t == W.FLOAT64:
        out = values.view(np.uint64).tolist()
    elif t == W.BOOL:
        out = np.unpackbits(values, bitorder="little")[c.value_bit:c.value_bit + n].astype(bool).tolist()
    else:
        raw = values.tobytes()
        out = [raw[int(offsets[r]):int(offsets[r + 1])] for r in range(n)]
    return [v if p else None for v, p in zip(out, present.tolist())]


def type_of(c: Column) -> int:
    if c.kind == _capi.OXH_COL_FIXED8:
        return W.INT64 if "int64" in str(c.values.dtype) else W.FLOAT64
    return {_capi.OXH_COL_BOOL: W.BOOL, _capi.OXH_COL_BYTES32: W.STRING, _capi.OXH_COL_BYTES64: W.STRING64}[c.kind]


# ---------------------------------------------------------------- floats
@pytest.mark.parametrize("form", FORMS)
def test_float_edge_table(ctx, form):
    """As one column, and repeated across the lanes of several waves beside an integer column. stats4[2] is the
    restatement's count of cells outside the exact path's stated domain."""
    _, stats = check(ctx, form, [b"x"], [W.FLOAT64], [EDGE_FLOATS], who="the table")
    assert stats[2] == sum(W.float_deferred(v) for v in EDGE_FLOATS) > 10
    n = 5 * WAVE + 7
    column = [None if r % 11 == 5 else EDGE_FLOATS[r % len(EDGE_FLOATS)] for r in range(n)]
    check(ctx, form, [b"x", b"k"], [W.FLOAT64, W.INT64], [column, list(range(n))], who="across lanes")
    check(ctx, form, [b"a", b"b", b"c"], [W.FLOAT64] * 3, [column, column[::-1], EDGE_FLOATS * 10 + EDGE_FLOATS[:n - 10 * len(EDGE_FLOATS)]],
          header=False, who="three float columns")


@pytest.mark.parametrize("form", FORMS)
def test_all_cells_deferred_and_none(ctx, form):
    n = GROUP + 3
    _, stats = check(ctx, form, [b"x"], [W.FLOAT64], [[(1e15 + 2 * k) * (-1) ** k for k in range(n)]], who="all deferred")
    assert stats[2] == n
    _, stats = check(ctx, form, [b"x"], [W.FLOAT64], [[k / 4 for k in range(n)]], who="none deferred")
    assert stats[2] == 0
    _, stats = check(ctx, form, [b"x", b"y"], [W.FLOAT64, W.FLOAT64], [[1e15] * n, [None] * n], who="deferred beside nulls")
    assert stats[2] == n and stats[3] == n


@pytest.mark.parametrize("form", FORMS)
def test_deferred_cells_at_the_wave_and_grid_edges(ctx, form):
    """Deferred cells at rows 0, 63, 64 and around the grid round, every other cell on the exact path: the slots are
    in row order whatever the launch order. A large case: its text is known without the restatement."""
    n = G + 2
    at = [0, WAVE - 1, WAVE, G - 1, G, G + 1]
    values = np.full(n, 0.5)
    values[at] = [1e15, 0.1 + 0.2, 5e-324, 1e16, -1.5e16, 1.7976931348623157e308]
    texts = [b"0.5"] * n
    for r, text in zip(at, [b"1000000000000000.0", b"0.30000000000000004", b"5e-324", b"1e16", b"-1.5e16", b"1.7976931348623157e308"]):
        texts[r] = text
    ints = np.arange(n, dtype=np.int64)
    want = b"".join(b"%s,%d\n" % (t, k) for k, t in enumerate(texts))
    cols = [Column(_capi.OXH_COL_FIXED8, n, values), Column(_capi.OXH_COL_FIXED8, n, ints)]
    check(ctx, form, [b"x", b"k"], [W.FLOAT64, W.INT64], None, header=False, cols=cols, want=(want, (len(want), 0, len(at), 0)), who="grid edges")


# ---------------------------------------------------------------- strings
@pytest.mark.parametrize("strings", [W.STRING, W.STRING64], ids=["BYTES32", "BYTES64"])
@pytest.mark.parametrize("form", FORMS)
def test_string_cells(ctx, form, strings):
    cells = [b"", None, b",", b'"', b"\n", b"\r", b"plain", b"\t", b"'", b"a,", b",a", b'a"', b'"a', b"\xff\x00\xfe"]
    cells += [b'"' * k for k in range(1, 6)]
    cells += [b"x" * k for k in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)]
    column = cells * 3
    check(ctx, form, [b"s", b"k"], [strings, W.INT64], [column, list(range(len(column)))], who="small cells")
    check(ctx, form, [b"s"], [strings], [column], who="one column")
    check(ctx, form, [b"s", b"k"], [strings, W.INT64], [column, list(range(len(column)))], sep=0x09, who="tabs")
    check(ctx, form, [b"s", b"k"], [strings, W.INT64], [column, list(range(len(column)))], quote=0x27, who="single quotes")


@pytest.mark.parametrize("form", FORMS)
def test_empty_strings_and_nulls_in_every_arrangement(ctx, form):
    n = 2 * WAVE + 5
    for validity, cells in (("auto", [b"" if r % 2 else None for r in range(n)]), ("none", [b""] * n), ("always", [None] * n),
                            ("always", [b""] * n)):
        cols = [K.host_column(W.STRING, cells, validity=validity), K.host_column(W.INT64, list(range(n)))]
        _, stats = check(ctx, form, [b"s", b"k"], [W.STRING, W.INT64], [cells, list(range(n))], cols=cols, who=("empty / null", validity))
        assert stats[1] == sum(c is not None for c in cells) and stats[3] == sum(c is None for c in cells)


@pytest.mark.parametrize("form", FORMS)
def test_long_cells(ctx, form):
    """Cells of kLongCell - 1, kLongCell, kLongCell + 1 and about 100 KB, plain, with a separator (quoted, nothing
    doubled) and with quotes (doubled, 64 bytes a step); a hazard at every byte position of a step; a quote as the
    last byte of a step and as the first byte of the next."""
    cells = []
    for n in (LONG - 1, LONG, LONG + 1, 100_003):
        body = bytes(97 + k % 26 for k in range(n))
        cells += [body, body[:n // 2] + b"," + body[n // 2 + 1:], body[:n // 3] + b'"' + body[n // 3 + 1:n - 1] + b'"',
                  b'"' * n if n < 1000 else body.replace(b"a", b'"')]
    base = bytes(65 + k % 26 for k in range(LONG + 2 * WAVE))
    for p in range(WAVE):
        at = LONG // 2 + p
        cells += [base[:at] + b'"' + base[at + 1:], base[:at] + b"\n" + base[at + 1:]]
    for at in (63, 64, 127, 128):
        cells += [base[:at] + b'"' + base[at + 1:], base[:at] + b'""' + base[at + 2:], base[:at] + b'"' + base[at + 1:at + 64] + b'"' + base[at + 65:]]
    cells += [None, b"", b"short"]
    keys = list(range(len(cells)))
    check(ctx, form, [b"k", b"s"], [W.INT64, W.STRING], [keys, cells], who="long cells, int32 offsets")
    check(ctx, form, [b"s", b"k"], [W.STRING64, W.INT64], [cells[:40], keys[:40]], header=False, misalign=5, who="long cells, int64 offsets")


@pytest.mark.parametrize("form", FORMS)
def test_a_sliced_string_column(ctx, form):
    """offsets[0] != 0: the bytes in front of the first cell are hazards that must not show."""
    cells = [b"first", None, b"", b"a,b", b"x" * (LONG + 3), b"last"]
    for t in (W.STRING, W.STRING64):
        cols = [K.host_column(t, cells, lead=b'garbage,"\n\r' * 9, nbit=3), K.host_column(W.BOOL, [True] * 6)]
        check(ctx, form, [b"s", b"b"], [t, W.BOOL], [cells, [True] * 6], cols=cols, who=("sliced", t))


# ---------------------------------------------------------------- bitmaps
@pytest.mark.parametrize("form", FORMS)
def test_bitmaps_at_every_bit_offset(ctx, form):
    n = WAVE + 9
    truth = [(r * 7 + r // 3) % 3 == 0 for r in range(n)]
    for bit in range(8):
        for name, cells in (("alternating", [None if r % 2 else truth[r] for r in range(n)]), ("all null", [None] * n), ("no nulls", truth)):
            for validity in (("none", "always") if name == "no nulls" else ("always",)):
                ints = [None if (r + bit) % 3 == 0 else r - 40 for r in range(n)]
                cols = [K.host_column(W.BOOL, cells, vbit=bit, nbit=(bit + 3) % 8, validity=validity), K.host_column(W.INT64, ints, nbit=7 - bit, validity="always")]
                check(ctx, form, [b"b", b"i"], [W.BOOL, W.INT64], [cells, ints], cols=cols, who=("bit offset", bit, name, validity))


# ---------------------------------------------------------------- rows
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_row_counts(ctx, form, n):
    names, types, cells = mixed(n, seed=n)
    _, stats = check(ctx, form, names, types, cells, who=("rows", n))
    check(ctx, form, names, types, cells, header=False, who=("rows, no header", n))
    if n == 0:
        assert stats == (len(b"i,f,b,s,big\n"), 0, 0, 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [G - 1, G, G + 1])
def test_the_grid_cap_with_one_int64_column(ctx, form, n):
    values = (np.arange(n, dtype=np.int64) * 7919 - 2 ** 31) * (1 - 2 * (np.arange(n, dtype=np.int64) % 2))
    want = b"v\n" + ("\n".join(map(str, values.tolist())) + "\n").encode()
    check(ctx, form, [b"v"], [W.INT64], None, cols=[Column(_capi.OXH_COL_FIXED8, n, values)], want=(want, (len(want), 0, 0, 0)), who=("grid cap", n))


@pytest.mark.parametrize("form", FORMS)
def test_a_wave_whose_span_just_fits_and_just_exceeds_the_lds_limit(ctx, form):
    """64 rows of one string column and no header: the wave's span is the whole file. kCsvwSpanLds bytes are
    assembled in LDS at once, one byte more in two runs of rows; both at several destination alignments."""
    per = SPAN // WAVE
    assert per * WAVE == SPAN and per < LONG
    for extra in (-1, 0, 1, 2):
        cells = [bytes(97 + (r + k) % 26 for k in range(per - 1)) for r in range(WAVE)]
        cells[17] = cells[17] + b"z" * extra if extra > 0 else cells[17][:len(cells[17]) + extra]
        for misalign in (0, 1, 15):
            got, _ = check(ctx, form, [b"s"], [W.STRING], [cells], header=False, misalign=misalign, who=("span", SPAN + extra, misalign))
            assert len(got) == SPAN + extra
    # two waves: the second one's span starts where the first one's ended, at an odd byte
    cells = [b"q" * (per - 1)] * WAVE + [b"r" * (per - 2)] * (WAVE - 1) + [b"s,s"]
    check(ctx, form, [b"odd"], [W.STRING], [cells], who="two spans")
    # one wave in several runs: quoted 300-byte rows, a long cell that ends a run, nulls, and rows of kLongCell bytes
    # and more whose cells are all shorter (their lanes write them straight to the output)
    cells = [b"a" * 300] * 20 + [b"L" * (LONG + 88)] + [b"b," * 150] * 30 + [None, b""] + [b"c" * (LONG - 2)] * 11
    assert len(cells) == WAVE
    for misalign in (0, 3):
        check(ctx, form, [b"k", b"runs"], [W.INT64, W.STRING], [list(range(WAVE)), cells], misalign=misalign, who=("runs of rows", misalign))


@pytest.mark.parametrize("form", FORMS)
def test_one_column_and_fifty(ctx, form):
    n = GROUP + WAVE + 1
    ints = [[(r * 31 + c) * (-1) ** c if (r + c) % 17 else None for r in range(n)] for c in range(50)]
    check(ctx, form, [b"c%d" % c for c in range(50)], [W.INT64] * 50, ints, who="50 columns")
    check(ctx, form, [b"only"], [W.INT64], [ints[3]], who="1 column")


@pytest.mark.parametrize("form", FORMS)
def test_every_destination_alignment(ctx, form):
    names, types, cells = mixed(3 * WAVE + 5, seed=99)
    want = W.write(names, types, cells)
    for misalign in range(16):
        check(ctx, form, names, types, cells, misalign=misalign, want=want, who=("misalign", misalign))


# ---------------------------------------------------------------- header
@pytest.mark.parametrize("form", FORMS)
def test_headers(ctx, form):
    cells = [[1, 2, None], [b"x", b"", None], [True, False, True]]
    types = [W.INT64, W.STRING, W.BOOL]
    for names in ([b"a", b"b", b"c"], [b"a,b", b'say "hi"', b"two\nlines"], [b"", b"\r", b"\xc3\xa9"], [b"tab\there", b"b", b"c"]):
        for header in (True, False):
            for sep in (0x2C, 0x09):
                _, stats = check(ctx, form, names, types, cells, sep=sep, header=header, who=(names, header, sep))
                assert stats[1] == 1 + (sum(W.string_text(n, sep, 0x22)[1] for n in names) if header else 0)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("form", FORMS)
def test_refusals_in_the_headers_order(ctx, form):
    """Every OXH_ERR_INVALID that needs no device, alone and together with every later one, outputs untouched; then
    the ones the length pass finds; then the capacity one byte short, which writes nothing and reports the need."""
    call, where = K.check_refusals(form, ctx)
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    cells = [b"ab", b"c", b"def"]
    good = K.host_column(W.STRING, cells)
    backwards = good._replace(offsets=np.array([0, 2, 1, 4], dtype=np.int32))
    negative = good._replace(offsets=np.array([-1, 2, 3, 6], dtype=np.int32))
    for bad, what in ((backwards, b"offsets decrease"), (negative, b"negative")):
        c = K.Call(form, [bad, K.host_column(W.INT64, [1, 2, 3])], [W.STRING, W.INT64], [b"s", b"k"])
        size, stats = ctypes.c_uint64(77), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        assert c.run(ctx, None, 0, size=size, stats=stats) == _capi.OXH_ERR_INVALID and what in err(), err()
        assert size.value == 77 and list(stats) == [7] * 4
    if form == "device":   # the host form's own check finds it before a device is needed
        c = K.Call(form, [good._replace(values=None), K.host_column(W.INT64, [1, 2, 3])], [W.STRING, W.INT64], [b"s", b"k"])
        assert c.run(ctx, None, 0) == _capi.OXH_ERR_INVALID and b"bytes but no values" in err(), err()
    names, types, cells = mixed(WAVE + 1, seed=5)
    want, wstats = W.write(names, types, cells)
    c = K.Call(form, [K.host_column(t, col) for t, col in zip(types, cells)], types, names)
    if form == "device":
        import torch

        buf = torch.full((len(want) + K.PAD,), K.SENTINEL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        out = buf.data_ptr()
    else:
        buf = np.full(len(want) + K.PAD, K.SENTINEL, dtype=np.uint8)
        out = buf.ctypes.data
    assert c.run(ctx, out, len(want) - 1) == _capi.OXH_ERR_INVALID and b"the file has %d" % len(want) in err(), err()
    assert c.size == len(want) and c.stats == wstats
    raw = buf.cpu().numpy() if form == "device" else buf
    assert (raw == K.SENTINEL).all(), "a call with a short capacity wrote"
    assert c.run(ctx, out, len(want)) == _capi.OXH_OK and c.size == len(want)
    raw = buf.cpu().numpy() if form == "device" else buf
    same(raw[:len(want)].tobytes(), want, "exact capacity")


# ---------------------------------------------------------------- scratch
POISONED = {}   # form -> the first poison's outputs


@pytest.fixture(params=[0x00, 0xFF, 0x5A], ids=["0x00", "0xFF", "0x5A"])
def poison(request, ctx):
    L = _capi.lib()
    prev = L.oxh_set_scratch_poison(request.param)
    try:
        assert prev == -1, prev
        yield request.param
    finally:
        L.oxh_set_scratch_poison(-1)


@contextlib.contextmanager
def poisoned(what):
    L = _capi.lib()
    before = L.oxh_scratch_poisoned_bytes()
    yield
    assert L.oxh_scratch_poisoned_bytes() > before, (what, "no working allocation was poisoned")


@pytest.mark.parametrize("form", FORMS)
def test_outputs_do_not_depend_on_what_the_scratch_held(ctx, poison, form):
    names, types, cells = mixed(SCAN_TILE + WAVE + 3, seed=3)
    cells[3][5] = b"y" * (LONG + 100) + b'"'
    with poisoned("csv write"):
        got = check(ctx, form, names, types, cells, who=("poison", poison))
    assert got == POISONED.setdefault(form, got)


# ---------------------------------------------------------------- round trips
def device_frame(names, types, cells):
    return {n.decode(): K.to_device(K.host_column(t, c)) for n, t, c in zip(names, types, cells)}


def test_round_trip_on_the_device(ctx):
    """read_csv_device(write_csv_device(frame)) under the written types: integers, booleans and strings exactly, floats
    bit for bit but a NaN as the quiet NaN, nulls as nulls, empty strings as empty strings, the names as the names."""
    names, types, cells = mixed(GROUP + 7, seed=11)
    cells[1] = [v if v is None else EDGE_FLOATS[r % len(EDGE_FLOATS)] for r, v in enumerate(cells[1])]
    frame = device_frame(names, types, cells)
    text, stats = tabular.write_csv_device(frame, ctx=ctx, stream=ctx.stream, with_stats=True)
    want, wstats = W.write(names, types, cells)
    same(text.cpu().numpy().tobytes(), want, "write_csv_device")
    assert tuple(stats) == wstats
    back = tabular.read_csv_device(text, schema=[tabular.CSV_TYPE_NAMES[t] for t in types], ctx=ctx, stream=ctx.stream)
    assert list(back) == [n.decode() for n in names]
    for (name, c), t, column in zip(back.items(), types, cells):
        expect = [None if v is None else (K.to_bits(v) if v == v else 0x7FF8000000000000) for v in column] if t == W.FLOAT64 else column
        assert cells_of(c, t) == expect, name
    # a caller's capacity skips the measure; one byte short is the library's error
    again = tabular.write_csv_device(frame, ctx=ctx, capacity=len(want) + 100)
    same(again.cpu().numpy().tobytes(), want, "with a capacity")
    with pytest.raises(_capi.OxenError, match="the file has"):
        tabular.write_csv_device(frame, ctx=ctx, capacity=len(want) - 1)


def test_a_one_column_frame_loses_exactly_its_null_rows(ctx):
    """The stated limit: a null row of a one-column frame is an empty record, which the reader skips."""
    for t, cells in ((W.INT64, [1, None, 3, None, None, 6]), (W.STRING, [b"a", None, b"", None, b"c"]), (W.FLOAT64, [None, 0.5, None])):
        frame = device_frame([b"only"], [t], [cells])
        text = tabular.write_csv_device(frame, ctx=ctx)
        back = tabular.read_csv_device(text, schema=[tabular.CSV_TYPE_NAMES[t]], ctx=ctx)
        kept = [v if t != W.FLOAT64 else K.to_bits(v) for v in cells if v is not None]
        assert cells_of(back["only"], t) == kept and back["only"].nrows == len(kept)


@pytest.mark.parametrize("name", sorted(os.listdir(CSVS)))
def test_golden_files_read_write_read(ctx, name):
    """Each fixture is read, written, read again under the first read's types: the two reads are equal."""
    import torch

    data = open(os.path.join(CSVS, name), "rb").read()
    sep = "\t" if name.endswith(".tsv") or name == "tabs.csv" else ","
    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    first = tabular.read_csv_device(d_bytes, delimiter=sep, ctx=ctx, stream=ctx.stream)
    types = [type_of(c) for c in first.values()]
    text = tabular.write_csv_device(first, delimiter=sep, ctx=ctx, stream=ctx.stream)
    second = tabular.read_csv_device(text, delimiter=sep, schema=[tabular.CSV_TYPE_NAMES[t] for t in types], ctx=ctx, stream=ctx.stream)
    assert list(second) == list(first) and len(first) > 0
    lost = len(first) == 1
    for (n1, a), b, t in zip(first.items(), second.values(), types):
        want = cells_of(a, t)
        if lost:
            want = [v for v in want if v is not None]
        assert cells_of(b, t) == want, n1
    host = tabular.write_csv({n: Column(c.kind, c.nrows, *(None if x is None else x.cpu().numpy() for x in (c.values, c.offsets, c.validity)))
                              for n, c in first.items()}, delimiter=sep, ctx=ctx)
    assert host == text.cpu().numpy().tobytes()


def test_the_chain_over_a_fixture(ctx, tmp_path):
    """read_csv_device -> filter_rows_device -> take_device -> write_csv_device on mixed_data_types.csv, against the
    restatement applied to the taken columns on the host; then write_df of the same frame to a path."""
    import torch

    data = open(os.path.join(CSVS, "mixed_data_types.csv"), "rb").read()
    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    frame = tabular.read_csv_device(d_bytes, ctx=ctx, stream=ctx.stream)
    names, cols = list(frame), list(frame.values())
    terms, logical = tabular.filter_terms(frame, "is_correct == true || difficulty > 1")
    selected = tabular.filter_rows_device(cols, terms, logical, ctx=ctx)
    kept = tabular.take_device(cols, selected.idx, ctx=ctx)
    assert 0 < kept[0].nrows < cols[0].nrows
    text, stats = tabular.write_csv_device(dict(zip(names, kept)), ctx=ctx, stream=ctx.stream, with_stats=True)
    types = [type_of(c) for c in kept]
    plain = [[K.from_bits(v) if t == W.FLOAT64 and v is not None else v for v in cells_of(c, t)] for c, t in zip(kept, types)]
    want, wstats = W.write([n.encode() for n in names], types, plain)
    same(text.cpu().numpy().tobytes(), want, "the chain")
    assert tuple(stats) == wstats
    host_frame = {n: Column(c.kind, c.nrows, *(None if x is None else x.cpu().numpy() for x in (c.values, c.offsets, c.validity)))
                  for n, c in zip(names, kept)}
    path = tmp_path / "out.csv"
    assert tabular.write_df(host_frame, path, ctx=ctx) == want and path.read_bytes() == want
    tsv = tmp_path / "out.tsv"
    assert tabular.write_df(host_frame, tsv, ctx=ctx) == W.write([n.encode() for n in names], types, plain, sep=0x09)[0] == tsv.read_bytes()
