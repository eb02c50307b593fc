"""The concat (oxh_concat_columns_*, oxen_amd.tabular) without a GPU: the two entries are declared, exported and
bound at ABI version 5; every argument error comes back as OXH_ERR_INVALID, in the header's order, before
OXH_ERR_NODEVICE, and there is no CPU path; the host pieces in a program of their own, plain and under the
sanitizers; the restatement of tests/_concat.py pinned from outside by pyarrow's own concat of slices;
`slice_range` against a brute-force reading of polars' rule, `parse_slice` and `vstack` for their refusals."""
import ctypes
import subprocess

import numpy as np
import pytest

import _concat
import _take
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

FUNCTIONS = ["oxh_concat_columns_device", "oxh_concat_columns_host"]
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
VP = ctypes.c_void_p
FORMS = ["host", "device"]
NINES = 0x0909090909090909


def u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def u32(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def ptrs(*arrays):
    return (VP * len(arrays))(*[ctypes.cast(a, VP).value if a is not None else None for a in arrays])


def test_the_two_functions_are_declared_exported_and_bound(built_lib):
    assert set(FUNCTIONS) <= set(_capi.header_symbols())
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    assert [s for s in _capi.header_symbols() if "concat_columns" in s] == FUNCTIONS
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert len(_capi.SIGNATURES["oxh_concat_columns_device"][1]) == 18 and len(_capi.SIGNATURES["oxh_concat_columns_host"][1]) == 17
    assert f"#define OXH_CONCAT_MAX_PARTS {_capi.OXH_CONCAT_MAX_PARTS}" in open(_capi.HEADER).read()
    import oxen_amd

    for name in ("concat", "concat_device", "slice_range", "parse_slice", "slice_rows", "slice_rows_device", "head", "head_device",
                 "tail", "tail_device", "page", "page_device", "vstack", "vstack_device"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name


class Call:
    """A well-formed call as the raw ABI takes it: two parts of an Int32, a Boolean and a BYTES32 column, of 3
    and 2 rows; rows [1, 3) of the first and [0, 2) of the second. The outputs hold sentinels."""

    def __init__(self):
        self.ints = [(ctypes.c_int32 * 3)(1, 2, 3), (ctypes.c_int32 * 2)(4, 5)]
        self.bools = [(ctypes.c_uint8 * 1)(0b101), (ctypes.c_uint8 * 1)(0b10)]
        self.text = [ctypes.create_string_buffer(b"abcdef", 6), ctypes.create_string_buffer(b"xyz", 3)]
        self.off = [(ctypes.c_int32 * 4)(1, 3, 3, 6), (ctypes.c_int32 * 3)(0, 1, 3)]
        self.valid = (ctypes.c_uint8 * 1)(0b011)
        self.v = [(ctypes.c_uint64 * 8)(*[NINES] * 8) for _ in range(3)]      # 8-byte aligned
        self.n = [(ctypes.c_uint64 * 1)(NINES) for _ in range(3)]
        self.o2 = (ctypes.c_int32 * 5)(*[9] * 5)
        self.value_bytes, self.written = u64(7, 7, 7), u32(7)
        self.good = dict(nparts=2, ncols=3, kinds=u32(4, 16, 32), values=self.values(), offsets=self.offsets(),
                         validity=ptrs(None, self.valid, None, None, None, None), bits=u64(*[0] * 12), rows=u64(3, 2),
                         first=u64(1, 0), count=u64(2, 2), capacity=u64(0, 0, 64), out_values=ptrs(*self.v),
                         out_offsets=ptrs(None, None, self.o2), out_validity=ptrs(*self.n), value_bytes=self.value_bytes,
                         written=self.written)

    def values(self, **change):
        cells = {0: self.ints[0], 1: self.bools[0], 2: self.text[0], 3: self.ints[1], 4: self.bools[1], 5: self.text[1]}
        return ptrs(*[{**cells, **{int(k[1:]): v for k, v in change.items()}}[i] for i in range(6)])

    def offsets(self, p0="same", p1="same"):
        return ptrs(None, None, self.off[0] if p0 == "same" else p0, None, None, self.off[1] if p1 == "same" else p1)

    def untouched(self):
        return all(list(a) == [NINES] * len(a) for a in self.v + self.n) and list(self.o2) == [9] * 5 and \
            list(self.value_bytes) == [7, 7, 7] and list(self.written) == [7]

    def __call__(self, form, **change):
        a = {**self.good, **change}
        args = [None, a["nparts"], a["ncols"], a["kinds"], a["values"], a["offsets"], a["validity"], a["bits"], a["rows"], a["first"],
                a["count"], a["capacity"], a["out_values"], a["out_offsets"], a["out_validity"], a["value_bytes"], a["written"]]
        L = _capi.lib()
        return L.oxh_concat_columns_host(*args) if form == "host" else L.oxh_concat_columns_device(*args, None)


def past_the_argument_checks(rc):
    """What a well-formed call with a NULL context gives: OXH_ERR_NODEVICE where there is no device, and the
    NULL context's own OXH_ERR_INVALID where there is one."""
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in _capi.lib().oxh_last_error()


@pytest.mark.parametrize("form", FORMS)
def test_concat_argument_errors_need_no_device(built_lib, form):
    """Each of these is OXH_ERR_INVALID whether or not a device is there, with a NULL context; the order of
    the checks is the header's."""
    c = Call()
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    top = (1 << 32) - 2
    for table in ("kinds", "values", "offsets", "validity", "bits", "rows", "first"):          # NULL table arrays
        assert c(form, **{table: None}) == INVALID and b"is NULL" in err(), table
    assert c(form, nparts=0) == INVALID and b"nparts or ncols" in err()
    assert c(form, ncols=0) == INVALID and b"nparts or ncols" in err()
    assert c(form, nparts=_capi.OXH_CONCAT_MAX_PARTS + 1) == INVALID and b"OXH_CONCAT_MAX_PARTS" in err()
    assert c(form, kinds=u32(4, 33, 32)) == INVALID and b"unknown kind" in err()
    assert c(form, count=u64(3, 2)) == INVALID and b"part 0: first + count" in err()
    assert c(form, first=u64(1, 1)) == INVALID and b"part 1: first + count" in err()
    assert c(form, first=u64(1, (1 << 64) - 1)) == INVALID and b"part 1: first + count" in err()
    assert c(form, rows=u64(3, top + 1)) == INVALID and b"2^32 - 2 rows" in err()
    assert c(form, rows=u64(top, top), first=u64(0, 0), count=u64(top, 1)) == INVALID and b"output rows" in err()
    assert c(form, value_bytes=None) == INVALID and b"value_bytes or written" in err()
    assert c(form, written=None) == INVALID and b"value_bytes or written" in err()
    assert c(form, offsets=c.offsets(p1=None)) == INVALID and b"part 1 column 2 is a byte column without offsets" in err()
    assert c(form, values=c.values(c3=None)) == INVALID and b"part 1 column 0 has no values" in err()
    assert c(form, values=c.values(c1=None)) == INVALID and b"part 0 column 1 has no values" in err()
    # the outputs: all three arrays or none; a capacity with them; every buffer a column needs
    assert c(form, out_values=None) == INVALID and b"some of" in err()
    assert c(form, out_offsets=None, out_validity=None) == INVALID and b"some of" in err()
    assert c(form, capacity=None) == INVALID and b"value_capacity" in err()
    assert c(form, out_offsets=ptrs(None, None, None)) == INVALID and b"out_offsets" in err()
    assert c(form, out_validity=ptrs(c.n[0], None, c.n[2])) == INVALID and b"out_validity" in err()
    assert c(form, out_values=ptrs(None, c.v[1], c.v[2])) == INVALID and b"out_values" in err()
    decreasing, negative = (ctypes.c_int32 * 4)(1, 3, 2, 6), (ctypes.c_int32 * 3)(-1, 1, 3)
    if form == "device":   # the bit-packed outputs are written a 64-row word at a time
        off_by = lambda a, k: ctypes.cast(ctypes.addressof(a) + k, VP)  # noqa: E731
        assert c(form, out_validity=ptrs(c.n[0], off_by(c.n[1], 4), c.n[2])) == INVALID and b"8-byte aligned" in err()
        assert c(form, out_values=ptrs(c.v[0], off_by(c.v[1], 1), c.v[2])) == INVALID and b"8-byte aligned" in err()
        assert past_the_argument_checks(c(form, out_values=ptrs(off_by(c.v[0], 1), c.v[1], off_by(c.v[2], 3))))  # not bit-packed
    else:                  # the host form reads the offsets of the taken ranges; the device form's are on the device
        assert c(form, offsets=c.offsets(p0=decreasing)) == INVALID and b"part 0 column 2: offsets decrease" in err()
        assert c(form, offsets=c.offsets(p1=negative)) == INVALID and b"negative" in err()
        assert c(form, values=c.values(c5=None)) == INVALID and b"bytes but no values" in err()
        assert c(form, offsets=c.offsets(p0=decreasing), out_validity=ptrs(None, c.n[1], c.n[2])) == INVALID and b"out_validity" in err()
        assert past_the_argument_checks(c(form, offsets=c.offsets(p0=(ctypes.c_int32 * 4)(9, 3, 3, 6))))   # outside the taken range
    # the order of the checks
    bad_kind = u32(4, 33, 32)
    assert c(form, kinds=None, nparts=0) == INVALID and b"is NULL" in err()
    assert c(form, nparts=0, kinds=bad_kind) == INVALID and b"nparts or ncols" in err()
    assert c(form, nparts=_capi.OXH_CONCAT_MAX_PARTS + 1, kinds=bad_kind) == INVALID and b"OXH_CONCAT_MAX_PARTS" in err()
    assert c(form, kinds=bad_kind, count=u64(9, 2)) == INVALID and b"unknown kind" in err()
    assert c(form, count=u64(9, 2), rows=u64(3, top + 1)) == INVALID and b"first + count" in err()
    assert c(form, rows=u64(3, top + 1), written=None) == INVALID and b"2^32 - 2 rows" in err()
    assert c(form, written=None, offsets=c.offsets(p0=None)) == INVALID and b"value_bytes or written" in err()
    assert c(form, offsets=c.offsets(p0=None), values=c.values(c0=None)) == INVALID and b"without offsets" in err()
    assert c(form, values=c.values(c0=None), out_values=None) == INVALID and b"has no values" in err()
    assert c.untouched()
    # well formed: past every check above, to the device question
    none = dict(capacity=None, out_values=None, out_offsets=None, out_validity=None)
    assert past_the_argument_checks(c(form))
    assert past_the_argument_checks(c(form, **none))                                           # sizes only
    assert past_the_argument_checks(c(form, first=None, count=None))                           # whole parts
    assert past_the_argument_checks(c(form, count=u64(2, 0), values=c.values(c3=None, c4=None, c5=None), offsets=c.offsets(p1=None)))
    # the most rows there may be (without the byte column: the host form reads the offsets of a taken range)
    assert past_the_argument_checks(c(form, ncols=2, rows=u64(top, 2), first=u64(0, 0), count=u64(top - 2, 2), **none))
    assert c.untouched()


def test_no_output_rows_is_ok_without_a_device(built_lib):
    """N == 0: OXH_OK after the argument checks, sizes 0; with outputs a byte column's offsets get their single
    0 -- host memory in the host form, so no device is needed for it."""
    c = Call()
    none = dict(capacity=None, out_values=None, out_offsets=None, out_validity=None)
    for form in FORMS:
        assert c(form, count=u64(0, 0), **none) == OK
        assert list(c.value_bytes) == [0, 0, 0] and list(c.written) == [0]
        assert c(form, rows=u64(0, 0), first=None, count=None, **none) == OK
        assert c(form, count=u64(0, 0), ncols=0, **none) == INVALID                # ... after the argument checks
        assert c(form, count=u64(0, 0), ncols=2) == OK                              # no byte column: nothing to write anywhere
        assert list(c.written) == [1]
    assert c("host", count=u64(0, 0)) == OK
    assert list(c.o2) == [0, 9, 9, 9, 9] and list(c.written) == [1] and list(c.value_bytes) == [0, 0, 0]
    assert all(list(a) == [NINES] * len(a) for a in c.v + c.n)
    assert c("host", count=u64(0, 0), out_offsets=ptrs(None, None, None)) == INVALID


def test_python_argument_checks_come_before_any_device_call(built_lib):
    import torch

    c = Call()
    for form in FORMS:
        assert past_the_argument_checks(c(form))
    assert c.untouched()
    a, b = column(np.arange(4, dtype=np.int64)), column(np.arange(3, dtype=np.int64))
    if not torch.cuda.is_available():   # there is no CPU path: the Python layer hands the status on
        for call in (lambda: tabular.concat([[a], [b]]), lambda: tabular.head({"a": a}, 2), lambda: tabular.vstack([{"a": a}, {"a": b}])):
            with pytest.raises(_capi.OxenError) as e:
                call()
            assert e.value.code == NODEVICE, e.value
    for call, what in ((lambda: tabular.concat([]), "at least one part"), (lambda: tabular.concat([[]]), "at least one part"),
                       (lambda: tabular.concat([[a], [column(np.zeros(3, dtype=np.int32))]]), "part 1 has other column kinds"),
                       (lambda: tabular.concat([[a, b]]), "columns of part 0 have one row count"),
                       (lambda: tabular.concat([[a], [b]], [(0, 1)]), "one .first, count. per part"),
                       (lambda: tabular.concat([[a], [b]], [(0, 1), (2, 2)]), r"part 1: rows \[2, 4\) of 3"),
                       (lambda: tabular.concat([[a]], [(-1, 1)]), "part 0: rows"),
                       (lambda: tabular.concat([[a]] * (_capi.OXH_CONCAT_MAX_PARTS + 1)), "OXH_CONCAT_MAX_PARTS"),
                       (lambda: tabular.slice_rows({"a": a, "b": b}, 0, 1), "one row count"),
                       (lambda: tabular.slice_rows({"a": a}, 0, -1), "not negative"),
                       (lambda: tabular.head({}, 1), "at least one column"),
                       (lambda: tabular.page({"a": a}, -1, 1), "not negative")):
        with pytest.raises(_capi.OxenError, match=what) as e:
            call()
        assert e.value.code == INVALID


def test_host_pieces_native_program(built_lib, tmp_path):
    """The argument checks in their stated order, the prefix table, the bit streams, the item lists and the host
    form's staging plan in a program of their own: as build.py builds it, and under -fsanitize=address,undefined.
    Nothing is loaded into python under a sanitizer."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.CONCAT_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    exe = str(tmp_path / "concat_columns_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.CONCAT_TEST_SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---------------------------------------------------------------- the restatement, pinned from outside
def arrow_frame(pa, n, seed):
    rng = np.random.default_rng(seed)
    mask = lambda: rng.random(n) < 0.3  # noqa: E731
    words = ["", "a", "bc", "déf", "x" * 17, "0123456789abcdef"]
    return [pa.array(rng.integers(-100, 100, n).astype(np.int8), mask=mask()),
            pa.array(rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32), mask=mask()),
            pa.array(rng.random(n), mask=mask()),
            pa.array(rng.random(n) < 0.5, mask=mask()),
            pa.array([words[i] for i in rng.integers(0, len(words), n)], type=pa.string(), mask=mask()),
            pa.array([words[i] for i in rng.integers(0, len(words), n)], type=pa.large_string()),
            pa.array(rng.integers(0, 9, n).astype(np.int64))]


def test_restatement_concats_as_pyarrow_concats_slices():
    """tests/_concat.py against pyarrow.concat_arrays of Array.slice: the parts are themselves slices, so their
    bit offsets are not multiples of 8 and their offsets do not start at 0."""
    pa = pytest.importorskip("pyarrow")
    frames = [arrow_frame(pa, n, seed) for seed, n in enumerate((23, 70, 9, 1))]
    cuts = [(3, 17), (5, 65), (1, 7), (0, 1)]                      # the slice each part is made of
    ranges = [(2, 11), (0, 65), (7, 0), (0, 1)]                    # the rows taken of each part; one empty
    sliced = [[a.slice(s, n) for a in f] for f, (s, n) in zip(frames, cuts)]
    parts = [[tabular._arrow_column(str(i), a) for i, a in enumerate(f)] for f in sliced]
    assert any(c.validity_bit % 8 for p in parts for c in p) and any(int(c.offsets[0]) for p in parts for c in p if c.offsets is not None)
    for use in (ranges, None):
        got = _concat.concat(parts, use)
        take = use if use is not None else [(0, n) for _, n in cuts]
        for i, t in enumerate(got):
            want = pa.concat_arrays([f[i].slice(s, n) for f, (s, n) in zip(sliced, take)])
            if t.kind in _take.FIXED:   # the cells in the Arrow array's own type
                valid = _take.bits(t.validity, 0, t.nrows).tolist()
                cells = [v if ok else None for v, ok in zip(t.values.view(want.type.to_pandas_dtype()).tolist(), valid)]
            else:
                cells = _take.pylist(t)
            assert cells == want.to_pylist(), i
            assert t.nrows == len(want) and t.validity.size == -(-t.nrows // 8)


def test_restatement_buffers_are_fully_defined_and_values_stay_under_nulls():
    a = Column(4, 3, np.array([7, 8, 9], dtype=np.int32), None, np.array([0b101], dtype=np.uint8))
    s = Column(32, 3, np.frombuffer(b"..abcdef", dtype=np.uint8), np.array([2, 4, 5, 8], dtype=np.int32), np.array([0b10100], dtype=np.uint8), 0, 2)
    b = Column(16, 3, np.array([0b0110100], dtype=np.uint8), None, None, 2, 0)
    (i, t, f) = _concat.concat([[a, s, b], [a, s, b]], [(1, 2), (0, 2)])
    assert i.values.view(np.int32).tolist() == [8, 9, 7, 8] and i.validity.tolist() == [0b0110]      # 8 sits under a null
    assert t.offsets.tolist() == [0, 1, 4, 6, 7] and t.values.tobytes() == b"cdefabc" and t.validity.tolist() == [0b0110]
    assert f.values.tolist() == [0b0110] and f.validity.tolist() == [0b1111]
    empty = _concat.concat([[a, s, b]], [(3, 0)])
    assert [x.nrows for x in empty] == [0, 0, 0] and empty[1].offsets.tolist() == [0] and empty[1].values.size == 0
    # the device form's reading of bad offsets: the cell of a bad pair has length 0; a bad span holds nothing
    bad = s._replace(offsets=np.array([2, 6, 5, 8], dtype=np.int32), validity=None)
    assert _concat.has_bad_offsets([[bad]]) and not _concat.has_bad_offsets([[bad]], [(2, 1)])
    (r,) = _concat.concat([[bad], [s]], device_reading=True)
    assert r.offsets.tolist() == [0, 4, 4, 6, 8, 9, 12] and r.values.tobytes() == b"abcdefabcdef"
    neg = s._replace(offsets=np.array([-1, 4, 5, 8], dtype=np.int32), validity=None)
    (r,) = _concat.concat([[neg], [s]], device_reading=True)
    assert r.offsets.tolist() == [0, 0, 0, 0, 2, 3, 6] and r.values.tobytes() == b"abcdef"
    with pytest.raises(AssertionError):
        _concat.concat([[bad]])


# ---------------------------------------------------------------- slice, head, tail, page, vstack
def test_slice_range_is_polars_slice_by_brute_force():
    """Over nrows 0..5, offsets -7..7 and lengths 0..7: the rows a negative offset counts from the end and the
    window [start, start + length) holds, read off one row at a time."""
    for nrows in range(6):
        for offset in range(-7, 8):
            for length in range(8):
                start = offset + nrows if offset < 0 else offset
                rows = [r for r in range(nrows) if start <= r < start + length]
                first, count = tabular.slice_range(nrows, offset, length)
                assert 0 <= first <= nrows and 0 <= count <= nrows - first, (nrows, offset, length)
                assert list(range(nrows))[first:first + count] == rows, (nrows, offset, length)
    assert tabular.slice_range(10, 0, 3) == (0, 3) and tabular.slice_range(10, -3, 3) == (7, 3)      # head, tail
    assert tabular.slice_range(2, -5, 4) == (0, 1)                                                  # the window starts before the frame
    with pytest.raises(_capi.OxenError, match="not negative"):
        tabular.slice_range(3, 0, -1)


def test_parse_slice_and_its_three_refusals():
    assert tabular.parse_slice("0..10") == (0, 10) and tabular.parse_slice("330..333") == (330, 333)
    assert tabular.parse_slice("+1..+2") == (1, 2)                     # what i64::from_str takes
    for text in ("5", "1..2..3", "a..b", "", "..", "0..", "..10", " 0..10", "0 ..10", "0..10 ", "0x1..3", "1.0..3", str(1 << 63) + ".." + str(1 << 64)):
        with pytest.raises(_capi.OxenError, match="expected two whole numbers") as e:
            tabular.parse_slice(text)
        assert e.value.code == INVALID
    for text in ("-5..3", "-1..-1", str(-(1 << 63)) + ".." + str((1 << 63) - 1)):
        with pytest.raises(_capi.OxenError, match="start must not be negative"):
            tabular.parse_slice(text)
    for text in ("0..0", "10..3", "3..-1"):
        with pytest.raises(_capi.OxenError, match="start must be less than end"):
            tabular.parse_slice(text)


def test_vstack_refusals_name_the_first_mismatch():
    a = {"x": column(np.arange(3, dtype=np.int64)), "y": column(["a", "b", None])}
    for frames, what in (([], "at least one frame"),
                         ([a, {"x": a["x"]}], r"frame 1 has column None where frame 0 has 'y' \(column 1\)"),
                         ([a, {"y": a["y"], "x": a["x"]}], r"frame 1 has column 'y' where frame 0 has 'x' \(column 0\)"),
                         ([a, a, {"x": a["x"], "z": a["y"]}], r"frame 2 has column 'z' where frame 0 has 'y' \(column 1\)"),
                         ([a, {"x": a["x"], "y": a["y"], "z": a["y"]}], r"frame 1 has column 'z' where frame 0 has None \(column 2\)"),
                         ([a, {"x": column(np.arange(3, dtype=np.int32)), "y": a["y"]}], "column 'x' of frame 1 has kind 4, of frame 0 8")):
        for call in (tabular.vstack, tabular.vstack_device):
            with pytest.raises(_capi.OxenError, match=what) as e:
                call(frames)
            assert e.value.code == INVALID
