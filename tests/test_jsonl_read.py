"""The JSON Lines reader on the GPU (oxh_jsonl_*, oxen_amd/csrc/jsonl_read.hip; oxen_amd.tabular): both forms
against the restatement of tests/_jsonl.py -- a sequential byte-by-byte state machine with int() / float() behind
the grammars -- for EXACT equality of the whole outputs: values, offsets, validity bytes with the bits past nrows
zero, stats8, stats4, the names and the inferred types, every output buffer followed by sentinels that must
survive. Every column is read twice, as its inferred type and as a string column. The edges (the lane, the
wave-instruction, the tile, the scan's tile, the carry kernels' round, the grid cap, the long-cell threshold) are
read from the sources and the hazards placed at each +- 1. The large case is built from known cells with numpy and
compared with those cells; the restatement parses only the small adversarial parts."""
import json
import os
import re
import struct

import numpy as np
import pytest

from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_jsonl_call", os.path.join(HERE, "_jsonl_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
J = K.J
F = K.load("_floatcases", os.path.join(HERE, "_floatcases.py"))
make_df_jsonl = K.load("make_df_jsonl", os.path.join(HERE, "golden", "make_df_jsonl.py"))

FORMS = K.FORMS
BS = chr(92)
U = BS + "u"
CSRC = os.path.join(os.path.dirname(os.path.abspath(tabular.__file__)), "csrc")
SOURCES = {name: open(os.path.join(CSRC, name)).read() for name in ("jsonl_read.hip", "jsonl_host.hpp", "csv_host.hpp", "keyed_diff.hip")}
LANE = 16                                     # bytes of one lane's load
WAVE = 64 * LANE                              # bytes of one wave-instruction
TILE = int(re.search(r"constexpr uint32_t kTileBytes = (\d+);", SOURCES["csv_host.hpp"]).group(1))
LONG = int(re.search(r"constexpr uint32_t kLongCell = (\d+);", SOURCES["csv_host.hpp"]).group(1))
SLOT = int(re.search(r"constexpr uint32_t kDeferSlot = (\d+);", SOURCES["csv_host.hpp"]).group(1))
SCAN_PER = int(re.search(r"constexpr uint32_t kScanPer = (\d+), kScanTile = 256 \* kScanPer;", SOURCES["keyed_diff.hip"]).group(1))
SCAN_TILE = 256 * SCAN_PER
CARRY_CHUNK = int(re.search(r"constexpr uint32_t kCarryChunk = (\d+);", SOURCES["jsonl_host.hpp"]).group(1))
CAP = int(re.search(r"unsigned cap_grid\(uint64_t groups\) \{ return \(unsigned\)std::min<uint64_t>\(std::max<uint64_t>\(groups, 1\), (\d+)\); \}",
                    SOURCES["jsonl_read.hip"]).group(1))
G = CAP * 256                                 # rows of one round of a lane-per-row kernel
ROUND = CAP * TILE                            # bytes of one round of the index kernels
CARRY_ROUND = 256 * CARRY_CHUNK * TILE        # bytes of one round of the carry kernels
assert TILE == 256 * LANE and "jsonl_lane_masks(base, t * kJlTileBytes + 16ull * threadIdx.x" in SOURCES["jsonl_read.hip"]
assert "kJlTileBytes = csv::kTileBytes" in SOURCES["jsonl_read.hip"] and "kJlLongCell = csv::kLongCell" in SOURCES["jsonl_read.hip"]


# ---------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("form", FORMS)
def test_the_data_test_fixture_reads_to_its_three_columns(ctx, form):
    data = open(make_df_jsonl.FIXTURE, "rb").read()
    got = K.read_and_check(ctx, form, data)
    assert got.names == [b"id", b"text", b"category"] and got.inferred == [J.INT64, J.STRING, J.STRING] and got.nrows == 2
    frame = tabular.read_jsonl(make_df_jsonl.FIXTURE, ctx=ctx)
    assert list(frame) == ["id", "text", "category"] and frame["id"].values.tolist() == [1, 1]
    assert frame["text"].values.tobytes() == b"I love itI hate it" and frame["text"].offsets.tolist() == [0, 9, 18]
    assert tabular.jsonl_shape(make_df_jsonl.FIXTURE, ctx=ctx) == (3, 2)
    assert tabular.jsonl_schema(make_df_jsonl.FIXTURE, ctx=ctx) == [("id", "Int64"), ("text", "String"), ("category", "String")]
    assert list(tabular.read_df(make_df_jsonl.FIXTURE, ctx=ctx)) == ["id", "text", "category"]


@pytest.mark.parametrize("form", FORMS)
def test_every_rule_once_at_every_misalignment(ctx, form):
    """The golden file's text: escapes, a surrogate pair, an escaped key, a repeated key, nested values, reordered
    and missing keys, blank lines, CRLF, malformed lines of every sort, a last line without a newline."""
    data = make_df_jsonl.rules_text()
    golden = {c["name"]: c for c in json.load(open(make_df_jsonl.OUT))["cases"]}
    for misalign in range(16):
        got = K.read_and_check(ctx, form, data, what=f"misalign {misalign}", misalign=misalign, infer_rows=2 if misalign % 2 else 10000)
        want = golden["rules, a window of 2" if misalign % 2 else "rules"]
        assert list(got.stats8) == want["stats8"] and [n.decode() for n in got.names] == want["names"]
        assert [J.TYPE_NAMES[t] for t in got.inferred] == want["types"]
    K.read_and_check(ctx, form, data, strings=J.STRING64, infer_rows=K.EVERY_ROW)


@pytest.mark.parametrize("form", FORMS)
def test_lines_records_and_blanks(ctx, form):
    cases = [b"\n", b"\n\n\n\n", b" \t\r\n\r\n  ", b"{}", b"{}\n", b"{}\n{}\n{ }\r\n", b'{"a":1}', b'{"a":1}\r\n{"a":2}\r\n', b'\n\n{"a":1}\n\n{"a":2}',
             b"x", b"x\n", b'{"a":1}\n' * 130, b"\xef\xbb\xbf" + b'{"a":1}\n{"a":2}\n', b"{}\n" * 70 + b'{"a":true}\n']
    for data in cases:
        got = K.read_and_check(ctx, form, data, what=repr(data[:40]))
        assert got.stats8[0] + got.stats8[4] == len(J.lines_of(data))


# ---------------------------------------------------------------- the hazards at the edges
def fill(start: int) -> bytes:
    """Exactly `start` bytes of whole lines in front of a hazard: a record where it fits, else a blank line."""
    if start == 0:
        return b""
    if start < 12:
        return b" " * (start - 1) + b"\n"
    return b'{"p":"' + b"f" * (start - 9) + b'"}\n'


def hazards():
    """name -> (line, the offset in the line of the byte to put on the edge)."""
    out = {}
    line = '{"a":"x","b":1}'
    out["a quote on the edge"] = (line, line.index('x"') + 1)
    out["a newline on the edge"] = (line, len(line))
    out["a colon on the edge"] = (line, line.index(":"))
    out["the last brace on the edge"] = (line, len(line) - 1)
    line = '{"a":"ab' + BS + '"cd","b":2}'
    out["an escaped quote straddling it"] = (line, line.index(BS) + 1)
    line = '{"a":"ab' + BS + BS + '","b":2}'
    out["an escaped backslash before the closing quote"] = (line, line.index(BS) + 2)
    for k in (1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, 3 * TILE, 3 * TILE + 1):
        line = '{"a":"x' + BS * k + '"' + ('y"' if k % 2 else "") + ',"b":[' + str(k) + "]}"
        out[f"a run of {k} backslashes that ends in a quote"] = (line, 7 + k)
    inner = ",".join('[{"k":[%d,"}]"]},{"q":"%s"}]' % (i, BS + '"') for i in range(2 * TILE // 24 + 40))
    line = '{"a":[' + inner + '],"b":{"c":[' + inner + "]}}"
    assert len(line) > 4 * TILE
    out["a long line whose depth changes on both sides"] = (line, len(line) // 2)
    line = '{"a":"xy' + U + "d83d" + U + 'de00z","b":3}'
    out["a surrogate pair straddling it"] = (line, line.index(U) + 6)
    line = '{"a":"' + "w" * (640 - 6) + U + "D83D" + U + 'DE00z","b":4}'   # its low half starts at byte 640 of the cell: a 64-byte step
    out["a surrogate pair in a long cell"] = (line, line.index(U) + 6)
    line = '{"a":"' + "v" * (LONG + 5) + BS + 'n","b":5}'
    out["an escape as the last bytes of a long cell"] = (line, line.index(BS) + 1)
    for n in (LONG - 1, LONG, LONG + 1):
        line = '{"a":"' + "u" * n + '","b":[' + "1," * (n // 2) + "1]}"
        out[f"plain cells of {n} bytes and about"] = (line, 6 + n)
    line = '{"a":"unclosed}\n{"a":"good","b":6}'
    out["a malformed line directly before a good one"] = (line, line.index("\n"))
    line = '{"a":[1,2}}\n{"a":"' + BS + '","b":7}\n{"a":"fine","b":8}'
    out["a stray bracket and an escaped closing quote stay on their lines"] = (line, line.index("\n"))
    return out


HAZARDS = hazards()


@pytest.mark.parametrize("name", list(HAZARDS))
def test_hazards_at_the_lane_wave_and_tile_edges(ctx, name):
    line, at = HAZARDS[name]
    tail = '\n{"a":"after","b":-1,"c":null}\n{"c":' + "9" * 25 + "}"
    k = 0
    for edge in (LANE, WAVE, TILE, 2 * TILE):
        for d in (-1, 0, 1):
            misalign = (5 * k + 3) % 16
            start = edge + d - misalign - at          # the byte lies at `edge + d` of the aligned space
            while start < 0:
                start += TILE
            data = fill(start) + (line + tail).encode()
            K.read_and_check(ctx, FORMS[k % 2], data, what=f"{name}: edge {edge} {d:+d}, misalign {misalign}", misalign=misalign)
            k += 1


# ---------------------------------------------------------------- the schema
@pytest.mark.parametrize("form", FORMS)
def test_names_the_window_and_the_counts(ctx, form):
    rows = ['{"a":1,"b":"x"}'] * 70
    rows[3] = '{"a":2,"b":"y","c":true}'                         # first appears inside the window
    rows[5] = '{"b":"z","a' + U + '0061":3,"a":4}'               # reordered; an escaped key that is a new name
    rows[9] = '{"a' + U + '0062c":5,"a":6}'
    rows[12] = '{"abc":7,"a":8}'                                 # the escaped key's plain spelling: one column
    rows[20] = '{"a":9,"a":10,"b":"r","b":"s"}'                  # repeated keys: the first wins
    rows[40] = '{"a":11,"late":[1,2],"b":"t","later":{"x":1}}'   # first appears after a window of 30: ignored
    rows[41] = '{"a":12,"b":"u",}'
    rows[69] = '{"d":null}'
    data = "\n".join(rows).encode()
    for window in (1, 4, 6, 30, 64, 65, 10000, K.EVERY_ROW):
        got = K.read_and_check(ctx, form, data, what=f"window {window}", infer_rows=window)
        assert got.stats8[3] == 1
    got = K.read(ctx, form, data, infer_rows=30)
    assert got.names == [b"a", b"b", b"c", b"aa", b"abc"] and got.stats8[6] == 3 and got.stats8[7] == 2
    got = K.read(ctx, form, data)
    assert got.names == [b"a", b"b", b"c", b"aa", b"abc", b"late", b"later", b"d"] and got.stats8[6] == 0


@pytest.mark.parametrize("form", FORMS)
def test_a_wide_record_with_its_keys_reordered(ctx, form):
    """Every key of a non-canonical row is compared with every name: 300 keys in reverse still read, and fast."""
    width = 300
    keys = ["k%03d" % c for c in range(width)]
    rows = ["{" + ",".join('"%s":%d' % (k, r * width + c) for c, k in enumerate(keys)) + "}" for r in range(3)]
    rows += ["{" + ",".join('"%s":%d' % (k, -c) for c, k in reversed(list(enumerate(keys)))) + "}" for _ in range(70)]
    data = ("\n".join(rows) + "\n").encode()
    got = K.read(ctx, form, data, cols=[0, width - 1], types=[J.INT64, J.INT64])
    assert got.stats8 == (73, 73, width, 0, 0, 70, 0, 0) and got.names == [k.encode() for k in keys]
    assert got.buffers[0][0].view(np.int64).tolist() == [0, width, 2 * width] + [0] * 70
    assert got.buffers[1][0].view(np.int64).tolist() == [width - 1, 2 * width - 1, 3 * width - 1] + [-(width - 1)] * 70


@pytest.mark.parametrize("form", FORMS)
def test_every_type_asked_of_every_value_kind(ctx, form):
    values = ['"text"', '"' + U + '00e9' + BS + 't"', '""', "0", "-0", "42", "9223372036854775807", "-9223372036854775808", "9223372036854775808",
              "1.0", "1e3", "-2.5E-3", "1e400", "-1e400", "1e-400", "0.1", "123456789012345678901234567890", "true", "false", "null", "[1,2]",
              '{"k":"v"}', "[}", "tru", "01", "1.", ".5", '"bad' + BS + 'x"', '"lone' + U + 'd800"', "'single'", "nul", "-", '"a" "b"']
    rows = ['{"v":%s,"w":%s}' % (v, values[(i + 7) % len(values)]) for i, v in enumerate(values)] + ['{"w":1}', '{"v":1,}']
    data = ("\n".join(rows) + "\n").encode()
    for t in (J.INT64, J.FLOAT64, J.BOOL, J.STRING, J.STRING64):
        K.read_and_check(ctx, form, data, what=J.TYPE_NAMES[t], cols=[0, 1, 1, 0], types=[t, t, J.STRING, J.STRING64])
    got = K.read(ctx, form, data, cols=[0], types=[J.FLOAT64])
    assert got.stats4[0].deferred >= 4


@pytest.mark.parametrize("form", FORMS)
def test_the_float_families_through_the_deferral(ctx, form):
    """The JSON-grammar subset of the CSV float families (no leading '+', no bare '.', no leading zeros): every
    cell bit for bit float()'s, the deferred ones counted."""
    texts = [t for family in F.reader_families().values() for t in family if J.NUMBER_RE.fullmatch(t)]
    texts = F.shuffled(texts)[:6000] + [b"1" + b"0" * 400, b"0." + b"0" * 400 + b"1", b"1e-400", b"-1e400", b"2" * (SLOT + 1), b"3" * SLOT + b".5"]
    assert len(texts) > 3000
    data = b"".join(b'{"f":' + t + b"}\n" for t in texts)
    got = K.read(ctx, form, data, cols=[0], types=[J.FLOAT64])
    bits = got.buffers[0][0].view(np.uint64)
    want = np.array([struct.unpack("<Q", struct.pack("<d", float(t)))[0] for t in texts], dtype=np.uint64)
    bad = np.nonzero(bits != want)[0]
    assert bad.size == 0, [(texts[i], hex(bits[i]), hex(want[i])) for i in bad[:5]]
    deferred = sum(J.parse_float(t)[1] for t in texts)
    assert got.stats4[0] == (0, 0, deferred, 8 * len(texts)) and 0 < deferred < len(texts)
    assert (np.unpackbits(got.buffers[0][2], bitorder="little")[:len(texts)] == 1).all()


# ---------------------------------------------------------------- past the grid cap and the scans' tiles
def filler(first: int, count: int):
    """`count` 16-byte lines {"a":1xxxxxxx }\\n of known cells, built with numpy."""
    block = np.frombuffer(b'{"a":10000000 }\n', dtype=np.uint8)
    out = np.tile(block, count).reshape(count, 16)
    digits = np.arange(first, first + count, dtype=np.int64) + 10_000_000
    for k in range(8):
        out[:, 12 - k] = 0x30 + (digits // 10 ** k) % 10
    return out.reshape(-1).tobytes(), digits


def filler_buffers(digits, col: int, t: int):
    n = digits.size
    ones = J.pack(np.ones(n, dtype=bool))
    if col == 0 and t == J.INT64:
        return J.Buffers(digits.astype(np.uint64), None, ones, (0, 0, 0, 8 * n))
    if col == 0:
        chars = np.zeros((n, 8), dtype=np.uint8)
        for k in range(8):
            chars[:, 7 - k] = 0x30 + (digits // 10 ** k) % 10
        return J.Buffers(chars.reshape(-1), (np.arange(n + 1, dtype=np.int64) * 8).astype(np.int32), ones, (0, 0, 0, 8 * n))
    return J.Buffers(np.zeros(0, np.uint8), np.zeros(n + 1, dtype=np.int32), J.pack(np.zeros(n, dtype=bool)), (n, 0, 0, 0))


def test_one_case_past_the_grid_cap_the_carry_round_and_the_scans_tile_loop(ctx):
    """More bytes than one round of the index kernels, of the carry kernels and of the scan's tile, and more rows
    than one round of a lane-per-row kernel, with every row in the window. At the byte edge: the end of a run of
    backslashes of three tiles, inside a line whose depth changes on both sides."""
    assert ROUND == CARRY_ROUND == SCAN_TILE * TILE
    run = 3 * TILE + 1
    nest = ",".join('[{"k":[%d]}]' % i for i in range(40))
    special = ('{"a":-5,"s":"x' + BS * run + '"y","n":[' + nest + ']}\n{"a":"oops\n{"a":7,"s":"' + U + 'd83d' + U + 'de00"}\n').encode()
    at = special.index(b'"y"')                                        # the escaped quote that ends the run
    before = (ROUND - at) // 16
    head, head_digits = filler(0, before)
    rest, rest_digits = filler(before, G + 300 - before)
    assert abs(len(head) + at + 9 - ROUND) < 32                       # at misalignment 9, as read below
    data = head + special + rest
    assert len(data) > ROUND + 3 * TILE and before + 3 + rest_digits.size > G
    p = J.parse(special, 1 << 62)
    assert p.names == [b"a", b"s", b"n"] and p.stats8[3] == 1
    for form in FORMS:
        got = K.read(ctx, form, data, misalign=9, infer_rows=K.EVERY_ROW, cols=[0, 0, 1, 2], types=[J.INT64, J.STRING, J.STRING, J.STRING])
        n = head_digits.size + 3 + rest_digits.size
        assert got.stats8 == (n, n, 3, 1, 0, 0, 0, 1) and got.names == p.names and got.inferred == [J.INT64, J.STRING, J.STRING]
        for k, (c, t) in enumerate(zip(got.cols, got.types)):
            want = K.splice([(filler_buffers(head_digits, c, t), head_digits.size), (J.column(p, c, t), 3),
                             (filler_buffers(rest_digits, c, t), rest_digits.size)])
            K.same_column(got, k, want, f"{form} selection {k}")


# ---------------------------------------------------------------- the round trip and the Python layer
def to_device(c):
    import torch

    move = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()  # noqa: E731
    return tabular.Column(c.kind, c.nrows, move(c.values), move(c.offsets), move(c.validity), c.value_bit, c.validity_bit)


def test_write_jsonl_device_then_read_jsonl_device_comes_back_bit_for_bit(ctx):
    rng = np.random.default_rng(3)
    n = 700
    strings = [None if r % 11 == 5 else bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8)) for r in range(n)]
    strings[0], strings[1], strings[2] = bytes(range(256)), b"", bytes(range(256)) * 3
    ints = rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    ints[:4] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1]
    floats = np.array([float(f"{rng.integers(1, 10 ** int(d))}e{int(rng.integers(-30, 30))}") for d in rng.integers(1, 18, size=n)])
    floats[:6] = [0.0, -0.0, 5e-324, 1.7976931348623157e308, 0.1 + 0.2, -2.5]
    special = {10: float("nan"), 11: float("inf"), 12: float("-inf")}
    for r, v in special.items():
        floats[r] = v
    int_valid, float_valid = rng.random(n) > 0.1, rng.random(n) > 0.1
    bools = rng.random(n) > 0.5
    host = {"s": tabular.column(strings), "i": tabular.column(ints, int_valid), "f": tabular.column(floats, float_valid), "b": tabular.column(bools)}
    text = tabular.write_jsonl_device({k: to_device(c) for k, c in host.items()}, ctx=ctx, stream=ctx.stream)
    assert text.cpu().numpy().tobytes() == tabular.write_jsonl(host, ctx=ctx)
    back = tabular.read_jsonl_device(text, ctx=ctx, stream=ctx.stream)
    assert list(back) == ["s", "i", "f", "b"]
    bits = lambda c: np.unpackbits(c.validity.cpu().numpy(), bitorder="little")[:n].astype(bool)  # noqa: E731
    assert bits(back["s"]).tolist() == [s is not None for s in strings]
    assert back["s"].values.cpu().numpy().tobytes() == host["s"].values.tobytes() and back["s"].offsets.cpu().numpy().tolist() == host["s"].offsets.tolist()
    assert (bits(back["i"]) == int_valid).all() and (back["i"].values.cpu().numpy()[int_valid] == ints[int_valid]).all()
    finite = float_valid & np.isfinite(floats)
    assert (bits(back["f"]) == finite).all() and not bits(back["f"])[[10, 11, 12]].any()      # NaN and the infinities come back null
    assert (back["f"].values.cpu().numpy().view(np.uint64)[finite] == floats.view(np.uint64)[finite]).all()
    assert bits(back["b"]).all() and (np.unpackbits(back["b"].values.cpu().numpy(), bitorder="little")[:n].astype(bool) == bools).all()
    # the host form reads the same text to the same columns
    again = tabular.read_jsonl(text.cpu().numpy().tobytes(), ctx=ctx)
    for name in back:
        for field in ("values", "offsets", "validity"):
            a, b = getattr(back[name], field), getattr(again[name], field)
            assert (a is None) == (b is None) and (a is None or a.cpu().numpy().tobytes() == np.ascontiguousarray(b).tobytes()), (name, field)


def test_ignore_errors_both_ways(ctx, tmp_path):
    good = b'{"a":1,"b":"x"}\n{"a":2,"b":"y"}\n'
    malformed = good + b'{"a":3,}\n'
    unparsable = good + b'{"a":tru,"b":"z"}\n'
    for form_read in (tabular.read_jsonl, lambda data, **kw: tabular.read_jsonl_device(K.device_buffer(data, 3), **kw)):
        assert list(form_read(good, ctx=ctx)) == ["a", "b"]
        for data in (malformed, unparsable):
            with pytest.raises(_capi.OxenError, match="Could not read tabular data from path"):
                form_read(data, ctx=ctx)
            frame = form_read(data, ctx=ctx, ignore_errors=True)
            validity = frame["a"].validity if isinstance(frame["a"].validity, np.ndarray) else frame["a"].validity.cpu().numpy()
            assert validity.tolist() == [0b011] and frame["a"].nrows == 3
        # an unparsable cell in a column that is not selected raises nothing
        assert list(form_read(unparsable, ctx=ctx, columns=["b"])) == ["b"]
        assert list(form_read(good, ctx=ctx, schema={"a": "Float64"}, columns=["a"])) == ["a"]
    path = tmp_path / "x.ndjson"
    path.write_bytes(good)
    assert tabular.read_df(path, ctx=ctx)["a"].values.tolist() == [1, 2]


def device_chain(frame, ctx):
    """filter_rows_device -> take_device -> sort_indices_device -> take_device -> write_csv_device over device
    columns: the text, and the indices on the way."""
    names, cols = list(frame), list(frame.values())
    terms, logical = tabular.filter_terms(frame, "score > 0")
    selected = tabular.filter_rows_device(cols, terms, logical, ctx=ctx)
    kept = tabular.take_device(cols, selected.idx, ctx=ctx)
    perm, _ = tabular.sort_indices_device([kept[names.index("id")], kept[names.index("name")]], ctx=ctx)
    final = tabular.take_device(kept, perm, ctx=ctx)
    text = tabular.write_csv_device(dict(zip(names, final)), ctx=ctx, stream=ctx.stream)
    return text.cpu().numpy().tobytes(), selected.idx.cpu().numpy().tolist(), perm.cpu().numpy().tolist()


def test_the_chain_from_json_lines_equals_the_chain_from_csv(ctx):
    """read -> filter -> sort -> write_csv gives the same text whether the cells came from JSON Lines or from CSV:
    on the device, the Columns of read_jsonl_device and read_csv_device handed to the _device entries as they are,
    and once more through the host forms."""
    import torch

    rng = np.random.default_rng(8)
    n = 500
    ids, scores = rng.integers(0, 50, size=n), rng.integers(-1000, 1000, size=n)
    names = [f"name {int(v)}" for v in rng.integers(0, 30, size=n)]
    jsonl = "".join('{"id":%d,"score":%d,"name":"%s"}\n' % (i, s, m) for i, s, m in zip(ids, scores, names)).encode()
    csv = ("id,score,name\n" + "".join("%d,%d,%s\n" % (i, s, m) for i, s, m in zip(ids, scores, names))).encode()
    up = lambda data: torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")   # noqa: E731
    from_jsonl = device_chain(tabular.read_jsonl_device(up(jsonl), ctx=ctx, stream=ctx.stream), ctx)
    from_csv = device_chain(tabular.read_csv_device(up(csv), ctx=ctx, stream=ctx.stream), ctx)
    assert from_jsonl == from_csv
    assert from_jsonl[1] == np.nonzero(scores > 0)[0].tolist() and len(from_jsonl[2]) == len(from_jsonl[1])
    rows = sorted((int(i), m, int(s)) for i, s, m in zip(ids, scores, names) if s > 0)
    lines = from_jsonl[0].decode().splitlines()
    assert lines[0] == "id,score,name" and [(int(a), c) for a, b, c in (x.split(",") for x in lines[1:])] == [(i, m) for i, m, _ in rows]
    texts = []
    for frame in (tabular.read_jsonl(jsonl, ctx=ctx), tabular.read_csv(csv, ctx=ctx)):
        kept = tabular.filter_df(frame, "score > 0", ctx=ctx)
        kept = tabular.sort_by(tabular.sort_by(kept, "name", ctx=ctx), "id", ctx=ctx)
        texts.append(tabular.write_csv(kept, ctx=ctx))
    assert texts[0] == texts[1] == from_jsonl[0]
