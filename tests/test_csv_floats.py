"""The CSV float conversions on the GPU across the exact path: the reader's one IEEE multiply or divide by an entry of
kCsvPow10 (csv_fixed_kernel, csv_number.hpp) and the writer's nearbyint / divide / compare over kCsvwPow10 that its
length, list and emit kernels each make on their own (csv_write.hip, csv_text.hpp) are the two places of the tabular
code whose result depends on the device's arithmetic and code generation. The case families of tests/_floatcases.py go
through both forms here, in both row orders, for EXACT equality -- bits, bytes, validity, stats4 with the deferred
count, sentinels -- with what tests/_csv.py and tests/_csvwrite.py say of each cell (the functions of
tests/test_csv_floats_cpu.py, which also pins the families and the host build of the same headers): every power of ten
of both tables from both sides, m = 2^53 and e10 = +-22 and one past them, the ties of the multiplication, every
digit count in each of ryu's forms, exact and deferred cells side by side in a wave and past the grid round. Then the
two round trips on the device, and the integer texts at both ends of every digit count."""
import functools
import itertools

import numpy as np
import pytest

import _floatcases as F
import test_csv as tc
import test_csv_floats_cpu as cpu
import test_csv_write as tw
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column

pytestmark = pytest.mark.gpu

C, read, same_buffers = tc.C, tc.read, tc.same_buffers
K, W, check = tw.K, tw.W, tw.check
FORMS = ["host", "device"]
ORDERS = ["generated", "shuffled"]
G = max(tc.G, tw.G)                            # rows of one round of a lane-per-row kernel, the reader's and the writer's
assert tc.G == tw.G


# ---------------------------------------------------------------- the reader
def one_column(texts) -> bytes:
    return b"x\n" + b"\n".join(texts) + b"\n"


def as_strings(texts) -> C.Buffers:
    offsets = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offsets[1:])
    return C.Buffers(np.frombuffer(b"".join(texts), dtype=np.uint8), offsets.astype(np.int32), C.pack(np.ones(len(texts), bool)),
                     (0, 0, 0, int(offsets[-1])))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["R1", "R2", "R3", "R4", "R5", "all+R5"])
def test_reader_families_as_float64(ctx, form, name, order):
    """One one-column file per family and order, and all of them in one: the values' bits, the validity bytes (an R5
    cell is a null; the bits past the rows are zero), stats4 with the restatement's count of deferred cells, the
    sentinels behind every buffer."""
    texts = cpu.reader_texts(name, order)
    n, want = len(texts), cpu.reader_want(texts)
    got = read(ctx, form, one_column(texts), cols=[0], types=[C.FLOAT64])
    assert got.stats8 == (n + 1, n, 1, n + 1, 0, 0, 0, 0), got.stats8
    assert got.stats4[0][1] == (len([t for t in texts if t in F.R5]) if "R5" in name else 0)
    assert got.stats4[0][2] == want.stats4[2], ("deferred", got.stats4[0][2], want.stats4[2])
    same_buffers(got, 0, want, (form, name, order))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["all", "all+R5"])
def test_reader_families_under_inference(ctx, form, name):
    """Float64 when every cell is the grammar, String with R5 among them; the string column's bytes are the texts."""
    texts = cpu.reader_texts(name, "shuffled")
    type_ = C.FLOAT64 if name == "all" else C.STRING
    assert (name == "all") == all(cpu.read_cell(t) is not None for t in texts[:10000])
    got = read(ctx, form, one_column(texts))
    assert got.inferred == [type_] and got.cols == [0, 0] and got.types == [type_, C.STRING]
    same_buffers(got, 0, cpu.reader_want(texts) if name == "all" else as_strings(texts), (form, name, "as inferred"))
    same_buffers(got, 1, as_strings(texts), (form, name, "as strings"))


@pytest.mark.parametrize("form", FORMS)
def test_reader_deferred_values_land_in_their_rows(ctx, form):
    """The second column is the row number: a deferred value scattered to another row shows as a shift."""
    texts = cpu.reader_texts("all+R5", "shuffled")
    n = len(texts)
    data = b"x,k\n" + b"".join(b"%s,%d\n" % (t, r) for r, t in enumerate(texts))
    got = read(ctx, form, data, cols=[0, 1], types=[C.FLOAT64, C.INT64])
    assert got.stats8 == (n + 1, n, 2, 2 * (n + 1), 0, 0, 0, 0), got.stats8
    want = cpu.reader_want(texts)
    assert 0 < want.stats4[2] < n and want.stats4[1] > 0
    same_buffers(got, 0, want, (form, "floats beside row numbers"))
    same_buffers(got, 1, C.Buffers(np.arange(n, dtype=np.uint64), None, C.pack(np.ones(n, bool)), (0, 0, 0, 8 * n)), (form, "row numbers"))


# ---------------------------------------------------------------- the writer
def float_column_case(values, null_every=None):
    """(cols, (text, stats4)) of a FLOAT64 column beside an INT64 row-number column, from the cells' known texts."""
    n = len(values)
    texts, late = cpu.writer_want(values)
    gone = [null_every is not None and r % null_every == null_every - 1 for r in range(n)]
    want = b"x,k\n" + b"".join(b"%s,%d\n" % (b"" if g else t, r) for r, (t, g) in enumerate(zip(texts, gone)))
    stats = (len(want), 0, sum(d and not g for d, g in zip(late, gone)), sum(gone))
    cols = [K.host_column(W.FLOAT64, [None if g else v for v, g in zip(values, gone)]), Column(_capi.OXH_COL_FIXED8, n, np.arange(n, dtype=np.int64))]
    return cols, (want, stats)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "W4"])
def test_writer_families(ctx, form, name, order):
    """The whole text byte for byte, and stats4: the bytes, and the restatement's count of deferred cells."""
    cols, want = float_column_case(cpu.writer_values(name, order))
    assert (0 < want[1][2] < cols[0].nrows) and want[1][3] == 0
    check(ctx, form, [b"x", b"k"], [W.FLOAT64, W.INT64], None, cols=cols, want=want, who=(form, name, order))


@pytest.mark.parametrize("form", FORMS)
def test_writer_family_with_every_tenth_cell_null(ctx, form):
    values = cpu.writer_values("W1", "shuffled")
    cols, want = float_column_case(values, null_every=10)
    assert want[1][3] == len(values) // 10 and want[1][2] > 0
    check(ctx, form, [b"x", b"k"], [W.FLOAT64, W.INT64], None, cols=cols, want=want, who=(form, "W1 with nulls"))


@functools.lru_cache(maxsize=None)
def alternating_case(phase: int):
    """G + 66 rows of W2's and W3's cells, exact and deferred in turn from row to row (phase 0: the even rows exact):
    at rows 0, 63, 64 and G - 1, G, G + 1 -- the ends of the first wave and of the first grid round -- a cell of one
    kind sits between two of the other, and with both phases each of those rows is once exact and once deferred."""
    values = cpu.writer_values("W2") + cpu.writer_values("W3")
    texts, late = cpu.writer_want(values)
    kinds = [[(v, t) for v, t, d in zip(values, texts, late) if d == which] for which in (False, True)]
    assert min(len(k) for k in kinds) > 400
    n = G + 66
    cells = [kinds[(r + phase) & 1][(r >> 1) % len(kinds[(r + phase) & 1])] for r in range(n)]
    want = b"".join(b"%s,%d\n" % (t, r) for r, (_, t) in enumerate(cells))
    cols = [Column(_capi.OXH_COL_FIXED8, n, np.array([v for v, _ in cells], dtype=np.float64)), Column(_capi.OXH_COL_FIXED8, n, np.arange(n, dtype=np.int64))]
    return cols, (want, (len(want), 0, sum((r + phase) & 1 for r in range(n)), 0))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("phase", [0, 1])
def test_the_writers_three_decisions_agree(ctx, form, phase):
    """csvw_length_kernel, csvw_defer_list_kernel and the emit kernel each decide exact-or-deferred by their own call
    of float_form: where two of them disagree the length differs, the call reports kCsvwErrPlace, or the bytes are
    wrong. Text and stats only."""
    cols, want = alternating_case(phase)
    check(ctx, form, [b"x", b"k"], [W.FLOAT64, W.INT64], None, header=False, cols=cols, want=want, who=(form, "alternating", phase))


# ---------------------------------------------------------------- round trips on the device
def on_device(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def test_round_trip_bits_to_text_to_bits(ctx):
    """write_csv_device then read_csv_device over W1 to W4 as generated, then shuffled, behind the zeros, the NaNs
    and the infinities; two columns, so that no record is empty. Every finite double comes back with its bits (-0.0
    too), a NaN as the quiet NaN."""
    finite = [v for name in ("W1", "W2", "W3", "W4") for order in ORDERS for v in cpu.writer_values(name, order)]
    bits = np.concatenate([np.array(cpu.SPECIAL_BITS, dtype=np.uint64), np.array(finite, dtype=np.float64).view(np.uint64)])
    n = bits.size
    frame = {"x": Column(_capi.OXH_COL_FIXED8, n, on_device(bits.view(np.float64))), "k": Column(_capi.OXH_COL_FIXED8, n, on_device(np.arange(n, dtype=np.int64)))}
    text = tabular.write_csv_device(frame, ctx=ctx, stream=ctx.stream)
    back = tabular.read_csv_device(text, schema=["Float64", "Int64"], ctx=ctx, stream=ctx.stream)
    assert list(back) == ["x", "k"] and back["x"].nrows == n == back["k"].nrows
    want = np.where(np.isnan(bits.view(np.float64)), np.uint64(C.QUIET_NAN), bits)
    got = back["x"].values.cpu().numpy().view(np.uint64)
    differ = np.nonzero(got != want)[0]
    assert differ.size == 0, (differ.size, [(int(r), hex(int(got[r])), hex(int(want[r]))) for r in differ[:5]])
    for name in ("x", "k"):
        assert np.unpackbits(back[name].validity.cpu().numpy(), bitorder="little")[:n].all(), name
    assert np.array_equal(back["k"].values.cpu().numpy(), np.arange(n, dtype=np.int64))


def test_round_trip_text_to_bits_to_text(ctx):
    """The canonical texts of W1 to W3, repeated to G + 300 rows, as a file: read_csv_device then write_csv_device give
    the file's bytes back. Exact and deferred floats are in the second round of csv_fixed_kernel and of the writer's
    length and emit kernels."""
    import torch

    texts, late = [], []
    for name in ("W1", "W2", "W3"):
        t, d = cpu.writer_want(cpu.writer_values(name, "shuffled"))
        texts, late = texts + t, late + d
    n = G + 300
    assert len(texts) < n and {late[r % len(texts)] for r in range(G, n)} == {False, True}
    data = b"x\n" + b"\n".join(itertools.islice(itertools.cycle(texts), n)) + b"\n"
    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    frame = tabular.read_csv_device(d_bytes, schema=["Float64"], ctx=ctx, stream=ctx.stream)
    assert frame["x"].nrows == n
    out = tabular.write_csv_device(frame, ctx=ctx, stream=ctx.stream)
    tw.same(out.cpu().numpy().tobytes(), data, "text to bits to text")


# ---------------------------------------------------------------- integers
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ORDERS)
def test_integer_family_written_and_read(ctx, form, order):
    """digits_u64 and put_digits at both ends of every digit count 1..19 for both signs, and parse_int64 on the same
    texts: the writer's text and the reader's values, inference and string column against the restatements."""
    ints = F.integers() if order == "generated" else F.shuffled(F.integers())
    check(ctx, form, [b"v", b"k"], [W.INT64, W.INT64], [ints, list(range(len(ints)))], who=(form, "integers", order))
    check(ctx, form, [b"v"], [W.INT64], [ints], header=False, who=(form, "integers alone", order))
    got, _ = tc.check(ctx, form, b"v\n" + b"".join(b"%d\n" % v for v in ints), who=("integers", order))
    assert got.inferred == [C.INT64] and got.buffers[0][0].view(np.int64).tolist() == ints


def test_integer_family_round_trip_on_the_device(ctx):
    import torch

    ints = F.integers() + F.shuffled(F.integers())
    n = len(ints)
    frame = {"v": Column(_capi.OXH_COL_FIXED8, n, on_device(np.array(ints, dtype=np.int64))), "k": Column(_capi.OXH_COL_FIXED8, n, on_device(np.arange(n, dtype=np.int64)))}
    text = tabular.write_csv_device(frame, ctx=ctx, stream=ctx.stream)
    assert text.cpu().numpy().tobytes() == b"v,k\n" + b"".join(b"%d,%d\n" % (v, r) for r, v in enumerate(ints))
    back = tabular.read_csv_device(text, ctx=ctx, stream=ctx.stream)                    # the types are inferred
    assert list(back) == ["v", "k"] and back["v"].values.dtype == torch.int64 and back["v"].values.cpu().numpy().tolist() == ints
    assert np.unpackbits(back["v"].validity.cpu().numpy(), bitorder="little")[:n].all()
