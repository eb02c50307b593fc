"""The take of the joined rows' columns (oxh_take_columns_*, oxen_amd.tabular) without a GPU: the two
entries are declared, exported and bound at ABI version 5; every argument error comes back as
OXH_ERR_INVALID, in the header's order, before OXH_ERR_NODEVICE, and there is no CPU path; the restatement of
tests/_take.py is pinned from outside by pyarrow's `take` and `coalesce`; the column list of
`diff_contents` against hand-written lists derived from join_diff.rs:204-278 and diffs.rs:975-1007; the
host pieces in a program of their own."""
import ctypes
import subprocess

import numpy as np
import pytest

import _rowhash
import _take
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, column

FUNCTIONS = ["oxh_take_columns_device", "oxh_take_columns_host"]
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
VP = ctypes.c_void_p
FORMS = ["host", "device"]
NONE = _capi.OXH_TAKE_NULL


def u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def u32(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def ptrs(*arrays):
    return (VP * len(arrays))(*[ctypes.cast(a, VP).value if a is not None else None for a in arrays])


def test_the_two_functions_are_declared_exported_and_bound(built_lib):
    assert set(FUNCTIONS) <= set(_capi.header_symbols())
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    assert [s for s in _capi.header_symbols() if "take_columns" in s] == FUNCTIONS
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert len(_capi.SIGNATURES["oxh_take_columns_device"][1]) == 20 and len(_capi.SIGNATURES["oxh_take_columns_host"][1]) == 19
    hdr = open(_capi.HEADER).read()
    for name in ("OXH_TAKE_NULL", "OXH_TAKE_NO_COLUMN"):
        assert f"#define {name} 0xFFFFFFFF\n" in hdr and getattr(_capi, name) == 0xFFFFFFFF, name
    assert _capi.OXH_TAKE_NULL == _capi.OXH_KEYED_DIFF_NONE == _take.NONE   # the keyed diff's indices as it writes them
    import oxen_amd

    for name in ("take", "take_device", "diff_contents", "diff_dfs_contents", "output_columns", "columns_to_arrow"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert tabular.STATUS_COLUMN == "_oxen_diff_status"


class Call:
    """A well-formed call as the raw ABI takes it: an Int32 column of 3 rows, a Boolean of 3 and a BYTES32 of
    2; three output columns of 4 rows, the first with itself as the fallback through the other index array.
    The outputs hold sentinels."""

    def __init__(self):
        self.ints = (ctypes.c_int32 * 3)(1, 2, 3)
        self.bools = (ctypes.c_uint8 * 1)(0b101)
        self.text = ctypes.create_string_buffer(b"abcdef", 6)
        self.off = (ctypes.c_int32 * 3)(1, 3, 6)
        self.valid = (ctypes.c_uint8 * 1)(0b011)
        self.idx0, self.idx1 = u32(0, 2, NONE, 1), u32(1, NONE, 0, 0)
        self.v = [(ctypes.c_uint64 * 8)(*[0x0909090909090909] * 8) for _ in range(3)]      # 8-byte aligned
        self.n = [(ctypes.c_uint64 * 1)(0x0909090909090909) for _ in range(3)]
        self.o2 = (ctypes.c_int32 * 5)(*[9] * 5)
        self.value_bytes, self.written = u64(7, 7, 7), u32(7)
        self.good = dict(nsrc=3, kinds=u32(4, 16, 32), values=ptrs(self.ints, self.bools, self.text),
                         offsets=ptrs(None, None, self.off), validity=ptrs(None, self.valid, None), bits=u64(0, 0, 0, 0, 0, 0),
                         rows=u64(3, 3, 2), nout_rows=4, idx0=self.idx0, idx1=self.idx1, nout=3,
                         plan=u32(0, 0, 0, 1, 1, 0, NONE, 0, 2, 1, NONE, 0), capacity=u64(0, 0, 64),
                         out_values=ptrs(*self.v), out_offsets=ptrs(None, None, self.o2), out_validity=ptrs(*self.n),
                         value_bytes=self.value_bytes, written=self.written)

    def untouched(self):
        return all(list(a) == [0x0909090909090909] * len(a) for a in self.v + self.n) and list(self.o2) == [9] * 5 and \
            list(self.value_bytes) == [7, 7, 7] and list(self.written) == [7]

    def __call__(self, form, **change):
        a = {**self.good, **change}
        cast = lambda x: ctypes.cast(x, VP) if x is not None else None  # noqa: E731
        args = [None, a["nsrc"], a["kinds"], a["values"], a["offsets"], a["validity"], a["bits"], a["rows"], a["nout_rows"],
                cast(a["idx0"]), cast(a["idx1"]), a["nout"], a["plan"], a["capacity"], a["out_values"], a["out_offsets"],
                a["out_validity"], a["value_bytes"], a["written"]]
        L = _capi.lib()
        return L.oxh_take_columns_host(*args) if form == "host" else L.oxh_take_columns_device(*args, None)


def past_the_argument_checks(rc):
    """What a well-formed call with a NULL context gives: OXH_ERR_NODEVICE where there is no device, and the
    NULL context's own OXH_ERR_INVALID where there is one."""
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in _capi.lib().oxh_last_error()


@pytest.mark.parametrize("form", FORMS)
def test_take_argument_errors_need_no_device(built_lib, form):
    """Each of these is OXH_ERR_INVALID whether or not a device is there, with a NULL context; the order of
    the checks is the header's."""
    c = Call()
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    g = c.good
    for table in ("kinds", "values", "offsets", "validity", "bits", "rows", "plan"):          # NULL table arrays
        assert c(form, **{table: None}) == INVALID and b"is NULL" in err(), table
    assert c(form, nsrc=0) == INVALID and b"nsrc or nout" in err()
    assert c(form, nout=0) == INVALID and b"nsrc or nout" in err()
    assert c(form, kinds=u32(4, 33, 32)) == INVALID and b"unknown kind" in err()
    assert c(form, plan=u32(3, 0, 0, 1, 1, 0, NONE, 0, 2, 1, NONE, 0)) == INVALID and b"not there" in err()     # a >= nsrc
    assert c(form, plan=u32(0, 0, 3, 1, 1, 0, NONE, 0, 2, 1, NONE, 0)) == INVALID and b"not there" in err()     # b >= nsrc
    assert c(form, plan=u32(0, 2, 0, 1, 1, 0, NONE, 0, 2, 1, NONE, 0)) == INVALID and b"index array" in err()
    assert c(form, plan=u32(0, 0, 0, 2, 1, 0, NONE, 0, 2, 1, NONE, 0)) == INVALID and b"index array" in err()
    assert c(form, plan=u32(0, 0, 0, 1, 1, 0, 0, 0, 2, 1, NONE, 0)) == INVALID and b"kind differs" in err()    # Boolean, Int32 fallback
    assert c(form, nout_rows=(1 << 32) - 1) == INVALID and b"2^32 - 2" in err()
    assert c(form, rows=u64(3, (1 << 32) - 1, 2)) == INVALID and b"2^32 - 2" in err()
    assert c(form, value_bytes=None) == INVALID and b"value_bytes or written" in err()
    assert c(form, written=None) == INVALID and b"value_bytes or written" in err()
    assert c(form, offsets=ptrs(None, None, None)) == INVALID and b"without offsets" in err()
    assert c(form, values=ptrs(None, c.bools, c.text)) == INVALID and b"has no values" in err()
    if form == "host":   # the host form reads the offsets: the device form's are on the device
        assert c(form, offsets=ptrs(None, None, (ctypes.c_int32 * 3)(1, 0, 6))) == INVALID and b"decrease" in err()
        assert c(form, offsets=ptrs(None, None, (ctypes.c_int32 * 3)(-1, 3, 6))) == INVALID and b"negative" in err()
        assert c(form, values=ptrs(c.ints, c.bools, None)) == INVALID and b"bytes but no values" in err()
    # the outputs: all three arrays or none; a capacity with them; every buffer a column needs
    assert c(form, out_values=None) == INVALID and b"some of" in err()
    assert c(form, out_offsets=None, out_validity=None) == INVALID and b"some of" in err()
    assert c(form, capacity=None) == INVALID and b"value_capacity" in err()
    assert c(form, out_offsets=ptrs(None, None, None)) == INVALID and b"out_offsets" in err()
    assert c(form, out_validity=ptrs(c.n[0], None, c.n[2])) == INVALID and b"out_validity" in err()
    assert c(form, out_values=ptrs(None, c.v[1], c.v[2])) == INVALID and b"out_values" in err()
    if form == "device":   # the bit-packed outputs are written a 64-row word at a time
        off_by = lambda a, k: ctypes.cast(ctypes.addressof(a) + k, VP)  # noqa: E731
        assert c(form, out_validity=ptrs(c.n[0], off_by(c.n[1], 4), c.n[2])) == INVALID and b"8-byte aligned" in err()
        assert c(form, out_values=ptrs(c.v[0], off_by(c.v[1], 1), c.v[2])) == INVALID and b"8-byte aligned" in err()
        assert past_the_argument_checks(c(form, out_values=ptrs(off_by(c.v[0], 1), c.v[1], off_by(c.v[2], 3))))  # not bit-packed
    # the order of the checks
    bad_kind, bad_plan, bad_pair = u32(4, 33, 32), u32(3, 0, 0, 1, 1, 0, NONE, 0, 2, 1, NONE, 0), u32(0, 0, 0, 1, 1, 0, 0, 0, 2, 1, NONE, 0)
    assert c(form, kinds=None, nsrc=0, plan=bad_plan) == INVALID and b"is NULL" in err()
    assert c(form, nsrc=0, kinds=bad_kind, plan=bad_plan) == INVALID and b"nsrc or nout" in err()
    assert c(form, kinds=bad_kind, plan=bad_plan) == INVALID and b"unknown kind" in err()
    assert c(form, plan=bad_plan, nout_rows=1 << 33) == INVALID and b"not there" in err()
    assert c(form, plan=bad_pair, nout_rows=1 << 33) == INVALID and b"kind differs" in err()
    assert c(form, nout_rows=1 << 33, written=None) == INVALID and b"2^32 - 2" in err()
    assert c(form, written=None, offsets=ptrs(None, None, None)) == INVALID and b"value_bytes or written" in err()
    assert c(form, offsets=ptrs(None, None, None), out_values=None) == INVALID and b"without offsets" in err()
    assert c(form, values=ptrs(None, c.bools, c.text), out_values=None) == INVALID and b"has no values" in err()
    assert c.untouched()
    # well formed: past every check above, to the device question
    assert past_the_argument_checks(c(form))
    assert past_the_argument_checks(c(form, capacity=None, out_values=None, out_offsets=None, out_validity=None))   # sizes only
    assert past_the_argument_checks(c(form, idx0=None)) and past_the_argument_checks(c(form, idx1=None, idx0=None))
    assert past_the_argument_checks(c(form, rows=u64(3, 3, 0), offsets=ptrs(None, None, None)))   # a column without rows
    assert past_the_argument_checks(c(form, nout_rows=(1 << 32) - 2, rows=u64(3, (1 << 32) - 2, 2), capacity=None,
                                      out_values=None, out_offsets=None, out_validity=None))       # the most rows there may be
    assert c.untouched()
    assert g is c.good


def test_no_output_rows_is_ok_without_a_device(built_lib):
    """nout_rows == 0: OXH_OK after the argument checks, sizes 0; with outputs a byte column's offsets get
    their single 0 -- host memory in the host form, so no device is needed for it."""
    c = Call()
    none = dict(capacity=None, out_values=None, out_offsets=None, out_validity=None)
    for form in FORMS:
        assert c(form, nout_rows=0, **none) == OK
        assert list(c.value_bytes) == [0, 0, 0] and list(c.written) == [0]
        assert c(form, nout_rows=0, nsrc=0, **none) == INVALID                 # ... after the argument checks
        assert c(form, nout_rows=0, plan=u32(0, 0, NONE, 0, 1, 0, NONE, 0, 1, 1, NONE, 0), out_offsets=ptrs(None, None, None)) == OK
        assert list(c.written) == [1]                                            # no byte column: nothing to write anywhere
    assert c("host", nout_rows=0) == OK
    assert list(c.o2) == [0, 9, 9, 9, 9] and list(c.written) == [1] and list(c.value_bytes) == [0, 0, 0]
    assert all(list(a) == [0x0909090909090909] * len(a) for a in c.v + c.n)
    assert c("host", nout_rows=0, out_offsets=ptrs(None, None, None)) == INVALID


def test_no_cpu_path_for_the_take(built_lib):
    import torch

    c = Call()
    for form in FORMS:
        assert past_the_argument_checks(c(form))
    assert c.untouched()
    if not torch.cuda.is_available():   # the Python layer hands the status on
        with pytest.raises(_capi.OxenError) as e:
            tabular.take([np.arange(4, dtype=np.int64)], np.array([0, 1], dtype=np.uint32))
        assert e.value.code == NODEVICE, e.value
    with pytest.raises(_capi.OxenError, match="at least one index array"):
        tabular.take([np.arange(4, dtype=np.int64)], None)
    with pytest.raises(_capi.OxenError, match="one length"):
        tabular.take([np.arange(4, dtype=np.int64)], np.zeros(2, np.uint32), np.zeros(3, np.uint32))
    with pytest.raises(_capi.OxenError, match="plan entry"):
        tabular.take([np.arange(4, dtype=np.int64)], np.zeros(2, np.uint32), plan=[(1, 0, None, 0)])


def test_host_pieces_native_program(built_lib):
    """The argument checks, the staging plan of a column and the host form's output block, in a program of
    their own."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.TAKE_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---------------------------------------------------------------- the restatement, pinned from outside
def arrow_columns(pa, n, rng):
    null = lambda: rng.random(n) < 0.3  # noqa: E731
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, size=int(l))) + ("é" if l % 3 == 0 else "")
             for l in rng.integers(0, 12, size=n)]
    return {
        "i8": pa.array(rng.integers(-128, 128, size=n).tolist(), type=pa.int8(), mask=null()),
        "i32": pa.array(rng.integers(-2**31, 2**31, size=n).tolist(), type=pa.int32(), mask=null()),
        "i64": pa.array(rng.integers(-2**63, 2**63, size=n).tolist(), type=pa.int64(), mask=null()),
        "f64": pa.array(rng.standard_normal(n).tolist(), type=pa.float64(), mask=null()),
        "b": pa.array((rng.random(n) < 0.5).tolist(), type=pa.bool_(), mask=null()),
        "s": pa.array(words, type=pa.string(), mask=null()),
        "ls": pa.array(words, type=pa.large_string(), mask=null()),
        "nonull": pa.array(rng.integers(0, 100, size=n).tolist(), type=pa.int32()),
    }


def as_arrow(pa, taken, typ):
    """A `Taken` as a pyarrow array of type `typ`, over its buffers."""
    buf = lambda a: None if a is None else pa.py_buffer(np.ascontiguousarray(a).view(np.uint8))  # noqa: E731
    middle = [buf(taken.offsets)] if taken.offsets is not None else []
    return pa.Array.from_buffers(typ, taken.nrows, [buf(taken.validity)] + middle + [buf(taken.values)])


@pytest.mark.parametrize("start,length", [(0, 41), (3, 30), (13, 28), (1, 1)])
def test_restatement_takes_as_pyarrow_takes_and_coalesces(start, length):
    """Every kind, from arrays sliced at bit offsets 0, 3 and 13, with absent indices: the restatement's cells
    are `pyarrow.Array.take` with a null index, and with a fallback `pyarrow.compute.coalesce` of the two
    takes. Values are compared (to_pylist): pyarrow leaves the bytes under a null undefined."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.compute as pc

    rng = np.random.default_rng(100 + start)
    left = pa.table(arrow_columns(pa, 41, rng)).slice(start, length)
    right = pa.table(arrow_columns(pa, 37, rng)).slice(min(start, 5), 29 if length > 1 else 1)
    names = left.schema.names
    frame_l, frame_r = tabular.columns_from_arrow(left), tabular.columns_from_arrow(right)
    if start and length > 1:   # a slice keeps its offsets: nothing was rebased to bit 0
        assert frame_l["b"].value_bit == start and frame_l["s"].validity_bit == start
    sources = list(frame_l.values()) + list(frame_r.values())
    nout = 53
    i0 = rng.integers(0, left.num_rows, size=nout).astype(np.uint32)
    i1 = rng.integers(0, right.num_rows, size=nout).astype(np.uint32)
    i0[rng.random(nout) < 0.25] = NONE
    i1[rng.random(nout) < 0.25] = NONE
    as_index = lambda i: pa.array([None if v == NONE else int(v) for v in i], type=pa.uint32())  # noqa: E731
    k = len(names)
    # a plain take of every left column through idx0 and every right column through idx1 ...
    plain = _take.take(sources, i0, i1, [(c, 0, None, 0) for c in range(k)] + [(k + c, 1, None, 0) for c in range(k)])
    # ... the right column with the left as its fallback (the keys' coalesce), and the other way round
    fallback = _take.take(sources, i0, i1, [(k + c, 1, c, 0) for c in range(k)] + [(c, 0, k + c, 1) for c in range(k)])
    for c, name in enumerate(names):
        typ = left.schema.field(name).type
        want_l, want_r = left.column(name).combine_chunks().take(as_index(i0)), right.column(name).combine_chunks().take(as_index(i1))
        assert as_arrow(pa, plain[c], typ).to_pylist() == want_l.to_pylist(), name
        assert as_arrow(pa, plain[k + c], typ).to_pylist() == want_r.to_pylist(), name
        assert as_arrow(pa, fallback[c], typ).to_pylist() == pc.coalesce(want_r, want_l).to_pylist(), name
        assert as_arrow(pa, fallback[k + c], typ).to_pylist() == pc.coalesce(want_l, want_r).to_pylist(), name
        assert plain[c].kind == frame_l[name].kind
    # one array None: all absent
    only = _take.take(sources, None, i1, [(0, 0, k, 1), (0, 0, None, 0)])
    assert as_arrow(pa, only[0], pa.int8()).to_pylist() == right.column("i8").combine_chunks().take(as_index(i1)).to_pylist()
    assert _take.pylist(only[1]) == [None] * nout and not only[1].values.any() and not only[1].validity.any()


def test_restatement_buffers_are_fully_defined():
    """Zero under nulls, zero pad bits, offsets from 0, a null cell an empty span."""
    cols = [column(np.array([7, 8, 9], dtype=np.int32), validity=[True, False, True]),
            column(np.array([True, True, False])), column(["ab", None, "cde"])]
    i0 = np.array([2, 1, NONE, 0, 0], dtype=np.uint32)
    a, b, s = _take.take(cols, i0)
    assert a.values.view(np.int32).tolist() == [9, 0, 0, 7, 7] and a.validity.tolist() == [0b11001]
    assert b.values.tolist() == [0b11010] and b.validity.tolist() == [0b11011]
    assert s.offsets.dtype == np.int32 and s.offsets.tolist() == [0, 3, 3, 3, 5, 7] and s.values.tobytes() == b"cdeabab"
    assert s.validity.tolist() == [0b11001]
    assert _take.pylist(s) == ["cde", None, None, "ab", "ab"] and _take.pylist(b) == [False, True, None, True, True]
    signed = _take.take(cols, np.array([2, 1, -1, 0, 0], dtype=np.int64))      # KeyedDiff's -1 = absent
    assert all(np.array_equal(x.values, y.values) and np.array_equal(x.validity, y.validity) for x, y in zip(signed, (a, b, s)))
    empty = _take.take(cols, np.zeros(0, dtype=np.uint32))
    assert empty[2].offsets.tolist() == [0] and empty[0].values.size == 0 and empty[1].validity.size == 0


def test_columns_to_arrow_is_the_inverse_of_columns_from_arrow():
    pa = pytest.importorskip("pyarrow")
    table = pa.table(arrow_columns(pa, 41, np.random.default_rng(5)))
    for piece in (table, table.slice(8, 20), table.slice(3, 9).select(["b", "nonull"])):
        frame = tabular.columns_from_arrow(piece)
        back = tabular.columns_to_arrow(frame, piece.schema)
        assert back.schema == piece.schema and back.to_pylist() == piece.to_pylist()
    # over what a take returns: buffers at bit / offset 0
    frame = tabular.columns_from_arrow(table)
    taken = _take.take(list(frame.values()), np.array([5, NONE, 40, 0], dtype=np.uint32))
    cols = {name: Column(t.kind, t.nrows, t.values, t.offsets, t.validity) for name, t in zip(frame, taken)}
    want = table.take(pa.array([5, None, 40, 0], type=pa.uint32()))
    assert tabular.columns_to_arrow(cols, table.schema).to_pylist() == want.to_pylist()


# ---------------------------------------------------------------- the columns of `contents`
def names_of(left, right, keys, targets, display=()):
    frame = lambda names: {n: None for n in names}  # noqa: E731  (only the names matter)
    return tabular.output_columns(frame(left), frame(right), keys, targets, display)


LEFT, RIGHT = ["id", "name", "score", "note", "old"], ["name", "id", "note", "score", "new"]


def test_output_columns_with_keys_and_targets():
    """Keys in the right frame's order, coalesced right then left (join_diff.rs:95-102, :226-228); the targets
    in the right frame's order, both sides of an unchanged column (:230-239). The default display names
    (diffs.rs:985-1004: note.left, note.right, old.left, new.right) are no columns of the right frame, so
    `order_columns_by_schema` (:264-278) drops every one."""
    got = names_of(LEFT, RIGHT, ["id", "name"], ["score"])
    assert got == [("name", ("right", "name"), ("left", "name")), ("id", ("right", "id"), ("left", "id")),
                   ("score.left", ("left", "score"), None), ("score.right", ("right", "score"), None)]


def test_output_columns_with_keys_only():
    """The resolved targets are the unchanged columns that are not keys; they come in the right frame's order
    (note before score), whatever order they were resolved in."""
    assert tabular._keys_targets_smart_defaults({n: 0 for n in LEFT}, {n: 0 for n in RIGHT}, ["id"], []) == \
        (["id"], ["name", "score", "note"])
    got = names_of(LEFT, RIGHT, ["id"], ["name", "score", "note"])
    assert [g[0] for g in got] == ["id", "name.left", "name.right", "note.left", "note.right", "score.left", "score.right"]
    assert got[0] == ("id", ("right", "id"), ("left", "id")) and got[3] == ("note.left", ("left", "note"), None)


def test_output_columns_with_neither():
    """keys = every unchanged column, targets = the added and removed columns: `old` is no column of the
    right frame and is dropped; `new` is an added column and has only its right side (:231-232)."""
    keys, targets = tabular._keys_targets_smart_defaults({n: 0 for n in LEFT}, {n: 0 for n in RIGHT}, [], [])
    assert (keys, targets) == (["id", "name", "score", "note"], ["new", "old"])
    got = names_of(LEFT, RIGHT, keys, targets)
    assert [g[0] for g in got] == ["name", "id", "note", "score", "new.right"]
    assert got[-1] == ("new.right", ("right", "new"), None) and all(g[2] == ("left", g[0]) for g in got[:4])


def test_output_columns_with_a_target_on_one_side_only():
    """A target only the left frame has is dropped by `order_columns_by_schema` (the `.left` arm of :233-234 is
    never reached); one only the right frame has gives `.right`. A key only the right frame has is the right
    column alone; one only the left frame has is dropped."""
    got = names_of(LEFT, RIGHT, ["id"], ["old", "new", "score"])
    assert got == [("id", ("right", "id"), ("left", "id")), ("score.left", ("left", "score"), None),
                   ("score.right", ("right", "score"), None), ("new.right", ("right", "new"), None)]
    got = names_of(LEFT, RIGHT, ["new", "old", "id"], ["score"])
    assert got[:2] == [("id", ("right", "id"), ("left", "id")), ("new", ("right", "new"), None)] and len(got) == 4


def test_output_columns_display_names_survive_only_as_literal_right_columns():
    """A display name passes `order_columns_by_schema` only if the right frame has a column of that literal
    name; then its suffix is stripped (:242-257) and the side it names is taken."""
    right = RIGHT + ["note.left", "new.right", "old.left", "score.right", "ghost.left", "name.right.right"]
    display = ["note.left", "note.right", "new.right", "old.left", "score.right", "ghost.left", "new.left", "name.right.right"]
    got = names_of(LEFT, right, ["id"], ["name"], display)
    assert got[:3] == [("id", ("right", "id"), ("left", "id")), ("name.left", ("left", "name"), None),
                       ("name.right", ("right", "name"), None)]
    # in the right frame's order; note.right is no literal column; ghost is in no frame; trim_end_matches strips
    # every repetition of the suffix
    assert got[3:] == [("note.left", ("left", "note"), None), ("new.right", ("right", "new"), None),
                       ("old.left", ("left", "old"), None), ("score.right", ("right", "score"), None),
                       ("name.right.right", ("right", "name"), None)]
    # the same names against a right frame without those columns: nothing survives
    assert names_of(LEFT, RIGHT, ["id"], ["name"], display) == got[:3]
    # an empty display is the smart default, which names only suffixed columns
    assert names_of(LEFT, RIGHT + ["note.left"], ["id"], ["name", "score"]) == \
        names_of(LEFT, RIGHT + ["note.left"], ["id"], ["name", "score"], ["note.left", "note.right", "old.left", "new.right"])
    assert names_of(LEFT, RIGHT + ["note.left"], ["id"], ["name", "score"])[-1] == ("note.left", ("left", "note"), None)


def test_diff_contents_over_the_restatements(monkeypatch):
    """`diff_contents` with `take` answered by the restatement: the keys coalesced right then left, the
    sides through their own index array, the status column from STATUS_NAMES."""
    def fake_take(columns, idx0, idx1=None, plan=None, ctx=None):
        return [Column(t.kind, t.nrows, t.values, t.offsets, t.validity) for t in _take.take(columns, idx0, idx1, plan)]

    monkeypatch.setattr(tabular, "take", fake_take)
    left = {"id": column(np.array([1, 2, 3], dtype=np.int64), validity=[True, True, False]), "name": column(["a", "b", "c"]),
            "old": column(np.array([5, 6, 7], dtype=np.int32))}
    right = {"name": column(["B", None, "d"]), "id": column(np.array([2, 3, 4], dtype=np.int64))}
    d = tabular.KeyedDiff(np.array([0, 1, 2, -1]), np.array([-1, 0, 1, 2]), np.array([2, 3, 1, 1], dtype=np.uint8), 2, 1, 1, 0, 0, 0)
    contents = tabular.diff_contents(left, right, d, ["id"], ["name"])
    assert list(contents) == ["id", "name.left", "name.right", "_oxen_diff_status"]
    assert _take.pylist(contents["id"]) == [1, 2, 3, 4]                  # right, else left (left row 2's id is null: right's 3)
    assert _take.pylist(contents["name.left"]) == ["a", "b", "c", None]
    assert _take.pylist(contents["name.right"]) == [None, "B", None, "d"]
    assert _take.pylist(contents["_oxen_diff_status"]) == ["removed", "modified", "added", "added"]
    assert _rowhash.bits(contents["id"].validity, 0, 4).all()
