"""The JSON writer on the GPU (oxh_write_json_*, oxen_amd/csrc/json_write.hip; oxen_amd.tabular): both forms and both
formats against the restatement of tests/_jsonwrite.py -- a sequential cell-by-cell writer -- for EXACT equality of
the whole buffer, out_bytes and stats4, every output between sentinel bytes that must survive. The edges (rows per
wave and workgroup, the grid cap, the long-cell threshold, the scan's tile, the LDS span limit, the escaping step and
the point where its stage is stored) are read from the sources and the cases placed at every one of them +- 1. The large cases are built from known cells and compared with
their known text; the restatement writes only the small adversarial frames.

Not run at its size: the refusal of a single row whose text is 2^32 bytes or more (a cell of 4 GiB that one wave counts
512 bytes a step); the check itself (a u64 sum per row against 2^32 in both length kernels) is read, not run."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_jsonwrite_call", os.path.join(HERE, "_jsonwrite_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
J = K.J
T = K.C.load("_test_csv_write_helpers", os.path.join(HERE, "test_csv_write.py"))   # EDGE_FLOATS, cells_of, type_of
FORMS, FORMATS = K.FORMS, K.FORMATS
FORMAT_IDS = ["lines", "array"]
CSVS = os.path.join(HERE, "golden", "data_test", "csvs")
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("json_write.hip", "csv_text.hpp", "keyed_diff.hip")}
WAVE = 64                                     # rows of one wave: a lane per row
assert "const unsigned lane = threadIdx.x & 63" in SOURCES["json_write.hip"]
GROUP = int(re.search(r"const uint64_t i = t \* stride \+ \(uint64_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x;", SOURCES["json_write.hip"]).group(1))
CAP = int(re.search(r"constexpr unsigned kJsonwMaxGroups = (\d+);", SOURCES["json_write.hip"]).group(1))
SPAN = int(re.search(r"constexpr uint32_t kJsonwSpanLds = (\d+);", SOURCES["json_write.hip"]).group(1))
assert re.search(r"constexpr uint32_t kJsonwLongCell = csvtext::kLongCell;", SOURCES["json_write.hip"])
LONG = int(re.search(r"constexpr uint32_t kLongCell = (\d+);", SOURCES["csv_text.hpp"]).group(1))
STEP = int(re.search(r"constexpr uint32_t kJsonwEscapeStep = (\d+);", SOURCES["json_write.hip"]).group(1))   # source bytes of one escaping step
assert re.search(r"constexpr uint32_t kJsonwEscapeMost = 6 \* kJsonwEscapeStep;", SOURCES["json_write.hip"])
STAGE_KEEPS = SPAN + 16 - 6 * STEP            # staged bytes above which the next step is stored first
SCAN_PER = int(re.search(r"constexpr uint32_t kScanPer = (\d+), kScanTile = 256 \* kScanPer;", SOURCES["keyed_diff.hip"]).group(1))
SCAN_TILE = 256 * SCAN_PER
G = CAP * GROUP                               # rows of one round of a lane-per-row kernel
assert GROUP == 256 and LONG == 512
EDGE_FLOATS = T.EDGE_FLOATS
ALL_BYTES = bytes(range(256))


# ---------------------------------------------------------------- helpers
same = T.same


def check(ctx, form, fmt, names, types, cells, misalign=0, cols=None, want=None, who=None):
    """One frame in one form and format against the restatement (or against `want`, a large case's known text and
    stats)."""
    cols = cols if cols is not None else [K.host_column(t, c) for t, c in zip(types, cells)]
    got, stats = K.write(ctx, form, cols, types, names, fmt, misalign)
    text, wstats = want if want is not None else J.write(names, types, cells, fmt)
    assert stats == wstats, (who, "stats4", stats, wstats)
    same(got, text, who)
    return got, stats


def mixed(n, seed=1):
    """n rows of five columns of every type, with nulls, bytes to escape, non-finite and deferred floats."""
    rng = np.random.default_rng(seed)
    strings = [b"plain", b"", b"a,b", b'say "hi"', b"two\nlines", b"cr\rhere", b"\xc3\xa9t\xc3\xa9", b"back\\slash", b"\x00\x01\x1f\x7f", b"x" * 40]
    floats = [0.5, 12.25, 0.1 + 0.2, 1e15, -0.0, float("nan"), float("-inf"), 1e-7, 123.456, 5e-324]
    pick = rng.integers(0, 10, size=(n, 5)).tolist()
    null = (rng.random((n, 5)) < 0.12).tolist()
    ints = rng.integers(-10 ** 12, 10 ** 12, size=n).tolist()
    cells = [[None if null[r][0] else ints[r] if pick[r][0] else -(1 << 63) for r in range(n)],
             [None if null[r][1] else floats[pick[r][1]] for r in range(n)],
             [None if null[r][2] else pick[r][2] < 5 for r in range(n)],
             [None if null[r][3] else strings[pick[r][3]] for r in range(n)],
             [None if null[r][4] else strings[pick[r][4]] * (1 + pick[r][0] % 3) for r in range(n)]]
    return [b"i", b"f", b"b", b"s", b"big"], [J.INT64, J.FLOAT64, J.BOOL, J.STRING, J.STRING64], cells


def rows_text(rows, fmt):
    """The file of known row objects."""
    return b"[" + b",".join(rows) + b"]" if fmt == J.ARRAY else b"".join(r + b"\n" for r in rows)


# ---------------------------------------------------------------- rows
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_row_counts(ctx, form, fmt, n):
    names, types, cells = mixed(n, seed=n)
    got, stats = check(ctx, form, fmt, names, types, cells, who=("rows", n))
    if n == 0:
        assert (got, stats) == ((b"[]", (2, 0, 0, 0)) if fmt == J.ARRAY else (b"", (0, 0, 0, 0)))
        got, stats = check(ctx, form, fmt, [b'q"'], [J.STRING], [[]], who="no rows, a name to escape")
        assert stats[1] == 0


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [G - 1, G, G + 1])
def test_the_grid_cap_with_one_int64_column(ctx, form, fmt, n):
    """The second grid-stride round, and the last row's byte behind its '}'. A large case: its text is known."""
    values = (np.arange(n, dtype=np.int64) * 7919 - 2 ** 31) * (1 - 2 * (np.arange(n, dtype=np.int64) % 2))
    want = rows_text([b'{"v":%d}' % v for v in values.tolist()], fmt)
    got, _ = check(ctx, form, fmt, [b"v"], [J.INT64], None, cols=[Column(_capi.OXH_COL_FIXED8, n, values)], want=(want, (len(want), 0, 0, 0)),
                   who=("grid cap", n))
    assert got.endswith(b"}]" if fmt == J.ARRAY else b"}\n") and got.count(b"]") == (fmt == J.ARRAY)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_a_wave_whose_span_just_fits_and_just_exceeds_the_lds_limit(ctx, form, fmt):
    """64 rows of one string column: the wave's span is all the rows. kJsonwSpanLds bytes are assembled in LDS at
    once, one byte more in two runs of rows; both at several destination alignments."""
    per = SPAN // WAVE
    frame = len(b'{"s":""}\n')
    assert per * WAVE == SPAN and per < LONG
    for extra in (-1, 0, 1, 2):
        cells = [bytes(97 + (r + k) % 26 for k in range(per - frame)) for r in range(WAVE)]
        cells[17] = cells[17] + b"z" * extra if extra > 0 else cells[17][:len(cells[17]) + extra]
        for misalign in (0, 1, 15):
            got, _ = check(ctx, form, fmt, [b"s"], [J.STRING], [cells], misalign=misalign, who=("span", SPAN + extra, misalign))
            assert len(got) == SPAN + extra + (fmt == J.ARRAY)
    # two waves: the second one's span starts where the first one's ended, at an odd byte
    cells = [b"q" * (per - frame)] * WAVE + [b"r" * (per - frame - 1)] * (WAVE - 1) + [b's"s']
    check(ctx, form, fmt, [b"s"], [J.STRING], [cells], who="two spans")
    # one wave in several runs: 300-byte rows, a long cell that ends a run, cells that widen, nulls, and rows of
    # kLongCell bytes and more whose cells are all shorter (their lanes write them straight to the output)
    cells = [b"a" * 300] * 20 + [b"L" * (LONG + 88)] + [b"b\n" * 100] * 30 + [None, b""] + [b"c" * (LONG - 2)] * 10 + [b"\x02" * 200]
    assert len(cells) == WAVE
    for misalign in (0, 3):
        check(ctx, form, fmt, [b"k", b"runs"], [J.INT64, J.STRING], [list(range(WAVE)), cells], misalign=misalign, who=("runs of rows", misalign))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_rows_at_the_long_row_threshold(ctx, form, fmt):
    """Rows whose text is kLongCell - 1, kLongCell and kLongCell + 1 bytes between short rows: the run splitting and
    the switch to the lane path. Plain cells, and cells whose escapes make the length."""
    frame = len(b'{"s":""}\n')
    cells = []
    for d in (-1, 0, 1):
        body = LONG + d - frame
        cells += [b"m" * body, b"ab", b"\n" * (body // 2) + b"x" * (body % 2), b"", b"\x03" * (body // 6) + b"y" * (body % 6), None]
    cells = cells * 5
    _, stats = check(ctx, form, fmt, [b"s"], [J.STRING], [cells], who="long-row threshold")
    lens = sorted({len(J.cell_text(J.STRING, c)[0]) + frame - 2 for c in cells if c})
    assert {LONG - 1, LONG, LONG + 1} <= set(lens)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_every_destination_alignment(ctx, form, fmt):
    names, types, cells = mixed(3 * WAVE + 5, seed=99)
    cells[4][70] = b"\n".join([b"line %d" % k for k in range(120)])   # a long cell that widens
    cells[4][71] = b"\x01" * (2 * STEP + 40) + b"tail\n" * 300        # one whose staged text is stored in several parts
    want = J.write(names, types, cells, fmt)
    for misalign in range(16):
        check(ctx, form, fmt, names, types, cells, misalign=misalign, want=want, who=("misalign", misalign))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_one_column_and_fifty(ctx, form, fmt):
    n = GROUP + WAVE + 1
    ints = [[(r * 31 + c) * (-1) ** c if (r + c) % 17 else None for r in range(n)] for c in range(50)]
    check(ctx, form, fmt, [b"c%d" % c for c in range(50)], [J.INT64] * 50, ints, who="50 columns")
    check(ctx, form, fmt, [b"only"], [J.INT64], [ints[3]], who="1 column")


# ---------------------------------------------------------------- strings
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("strings", [J.STRING, J.STRING64], ids=["BYTES32", "BYTES64"])
@pytest.mark.parametrize("form", FORMS)
def test_string_cells(ctx, form, strings, fmt):
    cells = [b"", None, b",", b'"', b"\n", b"\r", b"plain", b"\t", b"'", b"\\", b"/", b"\x7f", b"\x08", b"\x0c", b"\x00", b"\x1f", b'a"', b'"a', b"\xff\x00\xfe",
             ALL_BYTES, ALL_BYTES[::-1]]
    cells += [b'"' * k for k in range(1, 6)] + [b"\x01" * k for k in range(1, 4)]
    cells += [b"x" * k for k in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)]
    column = cells * 3
    _, stats = check(ctx, form, fmt, [b"s", b"k"], [strings, J.INT64], [column, list(range(len(column)))], who="small cells")
    assert stats[1] == 3 * sum(c is not None and J.string_text(c)[1] for c in cells)
    check(ctx, form, fmt, [b"s"], [strings], [column], who="one column")


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_long_cells(ctx, form, fmt):
    """Cells of kLongCell - 1 .. kLongCell + 65 source bytes, around two escaping steps and about 100 KB: plain
    (copied), and with escapes at byte 0, 63, 64, a step's last and first byte and the last byte of the cell; cells
    of only 0x01 (every byte six wide), one of them staged past the point where the stage is stored before the next
    step; widths cycling 1, 2, 6; all 256 byte values; an escape at every byte position around a lane's 8 bytes."""
    cells = []
    cycle = b"a\n\x01"
    assert STEP >= LONG and STAGE_KEEPS > 0 and 6 * 2 * STEP > STAGE_KEEPS   # a cell of 0x01 is stored before its third step
    for n in (LONG - 1, LONG, LONG + 1, LONG + 63, LONG + 64, LONG + 65, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1, 100_003):
        body = bytes(97 + k % 26 for k in range(n))
        cells.append(body)                                                      # nothing to escape
        for at in sorted({0, 63, 64, STEP - 1, STEP, n - 1} & set(range(n))):
            for esc in (b"\n", b"\x01"):
                cells.append(body[:at] + esc + body[at + 1:])
        cells.append(b'"' + body[1:63] + b"\\\t" + body[65:n - 1] + b"\x1f")     # all four places at once
        if n < 3 * STEP:
            cells += [b"\x01" * n, (cycle * (n // 3 + 1))[:n], (cycle[1:] + cycle[:1]) * (n // 3)]
    cells += [ALL_BYTES * 3, ALL_BYTES * 2 + b"tail", (ALL_BYTES + ALL_BYTES[::-1]) * 4]
    base = bytes(65 + k % 26 for k in range(LONG + 2 * WAVE))
    for p in range(WAVE):
        at = LONG // 2 + p
        cells += [base[:at] + b'"' + base[at + 1:], base[:at] + b"\x00" + base[at + 1:]]
    cells += [None, b"", b"short"]
    keys = list(range(len(cells)))
    _, stats = check(ctx, form, fmt, [b"k", b"s"], [J.INT64, J.STRING], [keys, cells], who="long cells, int32 offsets")
    assert stats[1] == sum(c is not None and J.string_text(c)[1] for c in cells)
    check(ctx, form, fmt, [b"s", b"k"], [J.STRING64, J.INT64], [cells[:60], keys[:60]], misalign=5, who="long cells, int64 offsets")


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_a_long_cell_in_a_null_row_and_a_sliced_column(ctx, form, fmt):
    """A null row whose offsets span a long cell full of bytes to escape: null, and nothing of the cell shows. Then
    offsets[0] != 0: the bytes in front of the first cell must not show."""
    hidden = [b"first", b"\n\x01" * LONG, b"", b'"' * (LONG + 3), b"last"]
    present = [True, False, True, False, True]
    for t in (J.STRING, J.STRING64):
        col = K.host_column(t, hidden)._replace(validity=K.C.packed(present, 5), validity_bit=5)
        cells = [c if p else None for c, p in zip(hidden, present)]
        _, stats = check(ctx, form, fmt, [b"s", b"b"], [t, J.BOOL], [cells, [True] * 5], cols=[col, K.host_column(J.BOOL, [True] * 5)], who=("null long cell", t))
        assert stats[1] == 0 and stats[3] == 2
    cells = [b"first", None, b"", b'a"b', b"x\n" * (LONG // 2 + 3), b"y" * (LONG + 3), b"last"]
    for t in (J.STRING, J.STRING64):
        cols = [K.host_column(t, cells, lead=b'garbage,"\n\r\x01' * 9, nbit=3), K.host_column(J.BOOL, [True] * 7)]
        check(ctx, form, fmt, [b"s", b"b"], [t, J.BOOL], [cells, [True] * 7], cols=cols, who=("sliced", t))


# ---------------------------------------------------------------- names
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_names(ctx, form, fmt):
    cells = [[1, 2, None], [b"x", b"", None], [True, False, True]]
    types = [J.INT64, J.STRING, J.BOOL]
    for names in ([b"a", b"b", b"c"], [b'q"b\\c\x01\n', "é€".encode(), b"/\x7f"], [b"", b"", b"\r"], [b"w" * 300, b"b", b"\x00" * 90]):
        _, stats = check(ctx, form, fmt, names, types, cells, who=names)
        assert stats[1] == sum(J.string_text(n)[1] for n in names)
    # 40 columns whose keys alone exceed kLongCell: every row is a long row, written by its lane
    names = [b"column_number_%02d" % c for c in range(40)]
    assert sum(len(n) + 4 for n in names) > LONG
    n = WAVE + 3
    ints = [[(r * 7 + c) if (r + c) % 5 else None for r in range(n)] for c in range(39)]
    strings = [b"s\n%d" % r if r % 3 else b"t" * (LONG + r) for r in range(n)]
    check(ctx, form, fmt, names, [J.INT64] * 39 + [J.STRING], ints + [strings], who="40 columns of long keys")


# ---------------------------------------------------------------- floats
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_float_edge_table(ctx, form, fmt):
    """As one column, and repeated across the lanes of several waves beside an integer column. The NaNs and the
    infinities are null and count in stats4[3]; stats4[2] is the cells outside the exact path's stated domain."""
    _, stats = check(ctx, form, fmt, [b"x"], [J.FLOAT64], [EDGE_FLOATS], who="the table")
    assert stats[2] == sum(J.float_deferred(v) for v in EDGE_FLOATS) > 10
    assert stats[3] == sum(math.isnan(v) or math.isinf(v) for v in EDGE_FLOATS) == 6
    n = 5 * WAVE + 7
    column = [None if r % 11 == 5 else EDGE_FLOATS[r % len(EDGE_FLOATS)] for r in range(n)]
    check(ctx, form, fmt, [b"x", b"k"], [J.FLOAT64, J.INT64], [column, list(range(n))], who="across lanes")
    check(ctx, form, fmt, [b"a", b"b", b"c"], [J.FLOAT64] * 3, [column, column[::-1], EDGE_FLOATS * 10 + EDGE_FLOATS[:n - 10 * len(EDGE_FLOATS)]],
          who="three float columns")


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_all_cells_deferred_and_none(ctx, form, fmt):
    n = GROUP + 3
    _, stats = check(ctx, form, fmt, [b"x"], [J.FLOAT64], [[(1e15 + 2 * k) * (-1) ** k for k in range(n)]], who="all deferred")
    assert stats[2] == n
    _, stats = check(ctx, form, fmt, [b"x"], [J.FLOAT64], [[k / 4 for k in range(n)]], who="none deferred")
    assert stats[2] == 0
    _, stats = check(ctx, form, fmt, [b"x", b"y"], [J.FLOAT64, J.FLOAT64], [[1e15] * n, [None] * n], who="deferred beside nulls")
    assert stats[2] == n and stats[3] == n


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_deferred_cells_at_the_wave_and_grid_edges(ctx, form, fmt):
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
    want = rows_text([b'{"x":%s,"k":%d}' % (t, k) for k, t in enumerate(texts)], fmt)
    cols = [Column(_capi.OXH_COL_FIXED8, n, values), Column(_capi.OXH_COL_FIXED8, n, ints)]
    check(ctx, form, fmt, [b"x", b"k"], [J.FLOAT64, J.INT64], None, cols=cols, want=(want, (len(want), 0, len(at), 0)), who="grid edges")


# ---------------------------------------------------------------- bitmaps
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_bitmaps_at_every_bit_offset(ctx, form, fmt):
    n = WAVE + 9
    truth = [(r * 7 + r // 3) % 3 == 0 for r in range(n)]
    for bit in range(8):
        for name, cells in (("alternating", [None if r % 2 else truth[r] for r in range(n)]), ("all null", [None] * n), ("no nulls", truth)):
            for validity in (("none", "always") if name == "no nulls" else ("always",)):
                ints = [None if (r + bit) % 3 == 0 else r - 40 for r in range(n)]
                cols = [K.host_column(J.BOOL, cells, vbit=bit, nbit=(bit + 3) % 8, validity=validity), K.host_column(J.INT64, ints, nbit=7 - bit, validity="always")]
                _, stats = check(ctx, form, fmt, [b"b", b"i"], [J.BOOL, J.INT64], [cells, ints], cols=cols, who=("bit offset", bit, name, validity))
                assert stats[3] == sum(c is None for c in cells) + sum(c is None for c in ints)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_all_rows_null_and_no_bitmap(ctx, form, fmt):
    n = 2 * WAVE + 5
    types = [J.INT64, J.FLOAT64, J.BOOL, J.STRING, J.STRING64]
    names = [b"i", b"f", b"b", b"s", b"S"]
    _, stats = check(ctx, form, fmt, names, types, [[None] * n] * 5, who="all rows null")
    assert stats[3] == 5 * n
    cells = [list(range(n)), [r / 8 for r in range(n)], [r % 3 == 0 for r in range(n)], [b"s%d" % r for r in range(n)], [b"" for r in range(n)]]
    cols = [K.host_column(t, c, validity="none") for t, c in zip(types, cells)]
    assert all(c.validity is None for c in cols)
    _, stats = check(ctx, form, fmt, names, types, cells, cols=cols, who="no bitmap")
    assert stats[3] == 0


# ---------------------------------------------------------------- calls
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_refusals_in_the_headers_order(ctx, form, fmt):
    """Every OXH_ERR_INVALID that needs no device, alone and together with every later one, outputs untouched; then
    the ones the length pass finds; then the capacity one byte short, which writes nothing and reports the need."""
    K.check_refusals(form, ctx, fmt)
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    good = K.host_column(J.STRING, [b"ab", b"c", b"def"])
    backwards = good._replace(offsets=np.array([0, 2, 1, 4], dtype=np.int32))
    negative = good._replace(offsets=np.array([-1, 2, 3, 6], dtype=np.int32))
    for bad, what in ((backwards, b"offsets decrease"), (negative, b"negative")):
        c = K.Call(form, [bad, K.host_column(J.INT64, [1, 2, 3])], [J.STRING, J.INT64], [b"s", b"k"], fmt)
        size, stats = ctypes.c_uint64(77), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        assert c.run(ctx, None, 0, size=size, stats=stats) == _capi.OXH_ERR_INVALID and what in err() and err().startswith(b"json write:"), err()
        assert size.value == 77 and list(stats) == [7] * 4
    if form == "device":   # the host form's own check finds it before a device is needed
        c = K.Call(form, [good._replace(values=None), K.host_column(J.INT64, [1, 2, 3])], [J.STRING, J.INT64], [b"s", b"k"], fmt)
        assert c.run(ctx, None, 0) == _capi.OXH_ERR_INVALID and b"bytes but no values" in err(), err()
    names, types, cells = mixed(WAVE + 1, seed=5)
    want, wstats = J.write(names, types, cells, fmt)
    c = K.Call(form, [K.host_column(t, col) for t, col in zip(types, cells)], types, names, fmt)
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
    assert c.run(ctx, out, len(want)) == _capi.OXH_OK and c.size == len(want) and c.stats == wstats
    raw = buf.cpu().numpy() if form == "device" else buf
    same(raw[:len(want)].tobytes(), want, "exact capacity")
    assert (raw[len(want):] == K.SENTINEL).all()


def test_the_python_layer_on_the_device(ctx, tmp_path):
    names, types, cells = mixed(GROUP + 7, seed=11)
    frame = {n.decode(): K.to_device(K.host_column(t, c)) for n, t, c in zip(names, types, cells)}
    host = {n.decode(): K.host_column(t, c) for n, t, c in zip(names, types, cells)}
    for fmt, device_fn, host_fn, ext in ((J.LINES, tabular.write_jsonl_device, tabular.write_jsonl, "jsonl"),
                                         (J.ARRAY, tabular.write_json_device, tabular.write_json, "json")):
        want, wstats = J.write(names, types, cells, fmt)
        text, stats = device_fn(frame, ctx=ctx, stream=ctx.stream, with_stats=True)
        same(text.cpu().numpy().tobytes(), want, device_fn.__name__)
        assert isinstance(stats, tabular.JsonWriteStats) and tuple(stats) == wstats
        again = device_fn(frame, ctx=ctx, capacity=len(want) + 100)
        same(again.cpu().numpy().tobytes(), want, "with a capacity")
        with pytest.raises(_capi.OxenError, match="the file has"):
            device_fn(frame, ctx=ctx, capacity=len(want) - 1)
        path = tmp_path / ("a." + ext)
        data, stats = host_fn(host, path, ctx=ctx, with_stats=True)
        assert data == want == path.read_bytes() and tuple(stats) == wstats
        path = tmp_path / ("b." + ext)
        assert tabular.write_df(host, path, ctx=ctx) == want == path.read_bytes()
    path = tmp_path / "c.ndjson"
    assert tabular.write_df(host, path, ctx=ctx) == J.write(names, types, cells, J.LINES)[0] == path.read_bytes()


# ---------------------------------------------------------------- the chain
def valid_utf8(raw: bytes) -> bool:
    try:
        raw.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.parametrize("name", sorted(os.listdir(CSVS)))
def test_golden_files_to_json(ctx, name):
    """Each fixture goes through read_csv_device, then write_jsonl_device and write_json_device: the text is the
    restatement's over the columns' cells, and for a file of valid UTF-8 json.loads of it gives the cells back."""
    import torch

    data = open(os.path.join(CSVS, name), "rb").read()
    sep = "\t" if name.endswith(".tsv") or name == "tabs.csv" else ","
    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    frame = tabular.read_csv_device(d_bytes, delimiter=sep, ctx=ctx, stream=ctx.stream)
    names, cols = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in frame], list(frame.values())
    types = [T.type_of(c) for c in cols]
    cells = [[K.from_bits(v) if t == J.FLOAT64 and v is not None else v for v in T.cells_of(c, t)] for c, t in zip(cols, types)]
    nrows = cols[0].nrows
    assert len(cols) > 0
    for fmt, fn in ((J.LINES, tabular.write_jsonl_device), (J.ARRAY, tabular.write_json_device)):
        text, stats = fn(frame, ctx=ctx, stream=ctx.stream, with_stats=True)
        got = text.cpu().numpy().tobytes()
        want, wstats = J.write(names, types, cells, fmt)
        same(got, want, (name, fmt))
        assert tuple(stats) == wstats
        if not valid_utf8(data):
            continue
        decoded = got.decode("utf-8")
        rows = [json.loads(line, object_pairs_hook=list) for line in decoded.split("\n")[:-1]] if fmt == J.LINES else json.loads(decoded, object_pairs_hook=list)
        assert len(rows) == nrows
        for r, row in enumerate(rows):
            assert [k for k, _ in row] == [n.decode("utf-8") for n in names]
            for c, (_, v) in enumerate(row):
                cell = cells[c][r]
                if cell is None or (types[c] == J.FLOAT64 and (math.isnan(cell) or math.isinf(cell))):
                    assert v is None
                elif types[c] == J.FLOAT64:
                    assert isinstance(v, float) and v == cell and math.copysign(1.0, v) == math.copysign(1.0, cell)
                elif types[c] in (J.STRING, J.STRING64):
                    assert v == cell.decode("utf-8")
                else:
                    assert v == cell and type(v) is type(cell)
