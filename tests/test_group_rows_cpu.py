"""The grouping of rows by equality on key columns (oxh_group_rows_*, oxen_amd.tabular) without a GPU: the two
entries are declared, exported and bound at ABI version 5; every argument error comes back as
OXH_ERR_INVALID, in the header's order, before OXH_ERR_NODEVICE, and there is no CPU path; the host pieces in a
program of their own, plain and under the sanitizers; the restatement of tests/_grouprows.py pinned to the
reference's recorded results (tests/golden/df_unique.json), and the compositions over the restatements."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import _grouprows
import _sortrows
import _take
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Column, GroupStats, RowGroups, column

FUNCTIONS = ["oxh_group_rows_device", "oxh_group_rows_host"]
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
VP = ctypes.c_void_p
FORMS = ["host", "device"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "df_unique.json")


def u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def u32(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def ptrs(*arrays):
    return (VP * len(arrays))(*[ctypes.cast(a, VP).value if a is not None else None for a in arrays])


def test_the_two_functions_are_declared_exported_and_bound(built_lib):
    assert set(FUNCTIONS) <= set(_capi.header_symbols())
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    assert [s for s in _capi.header_symbols() if "group_rows" in s] == FUNCTIONS
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert len(_capi.SIGNATURES["oxh_group_rows_device"][1]) == 15 and len(_capi.SIGNATURES["oxh_group_rows_host"][1]) == 14
    assert (_grouprows.SIGNED, _grouprows.UNSIGNED, _grouprows.FLOAT) == (_capi.OXH_SORT_SIGNED, _capi.OXH_SORT_UNSIGNED, _capi.OXH_SORT_FLOAT)
    import oxen_amd

    for name in ("RowGroups", "GroupStats", "group_rows", "group_rows_device", "unique", "unique_count", "is_duplicated", "n_duped_rows"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert tabular.RowGroups._fields == ("group", "count", "first_idx", "first_count", "stats")
    assert tabular.GroupStats._fields == ("groups", "duplicated", "largest", "long_rows")


class Call:
    """A well-formed call as the raw ABI takes it: three key columns of 3 rows -- Int32, Boolean, BYTES32.
    The outputs hold sentinels."""

    def __init__(self):
        self.ints = (ctypes.c_int32 * 3)(1, -2, 3)
        self.bools = (ctypes.c_uint8 * 1)(0b101)
        self.text = ctypes.create_string_buffer(b"abcdef", 6)
        self.off = (ctypes.c_int32 * 4)(1, 3, 3, 6)
        self.valid = (ctypes.c_uint8 * 1)(0b011)
        self.outs = [u32(9, 9, 9) for _ in range(4)]
        self.stats = u64(7, 7, 7, 7)
        self.good = dict(nrows=3, nkeys=3, kinds=u32(4, 16, 32), values=ptrs(self.ints, self.bools, self.text),
                         offsets=ptrs(None, None, self.off), validity=ptrs(None, self.valid, None), bits=u64(0, 0, 0, 0, 0, 0),
                         orders=u32(0, 0, 0), outs=self.outs, stats=self.stats)

    def untouched(self):
        return all(list(o) == [9, 9, 9] for o in self.outs) and list(self.stats) == [7, 7, 7, 7]

    def __call__(self, form, **change):
        a = {**self.good, **change}
        cast = lambda x: ctypes.cast(x, VP) if x is not None else None  # noqa: E731
        args = [None, a["nrows"], a["nkeys"], a["kinds"], a["values"], a["offsets"], a["validity"], a["bits"], a["orders"],
                *[cast(o) for o in a["outs"]], a["stats"]]
        L = _capi.lib()
        return L.oxh_group_rows_host(*args) if form == "host" else L.oxh_group_rows_device(*args, None)


def past_the_argument_checks(rc):
    """What a well-formed call with a NULL context gives: OXH_ERR_NODEVICE where there is no device, and the
    NULL context's own OXH_ERR_INVALID where there is one."""
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in _capi.lib().oxh_last_error()


@pytest.mark.parametrize("form", FORMS)
def test_group_argument_errors_need_no_device(built_lib, form):
    """Each of these is OXH_ERR_INVALID whether or not a device is there, with a NULL context; the order of
    the checks is the header's: the sort's list, then stats4, then the context."""
    c = Call()
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    for table in ("kinds", "values", "offsets", "validity", "bits", "orders"):          # NULL arrays
        assert c(form, **{table: None}) == INVALID and b"is NULL" in err() and b"group rows" in err(), table
    assert c(form, nkeys=0) == INVALID and b"nkeys is 0" in err()
    assert c(form, kinds=u32(4, 33, 32)) == INVALID and b"unknown kind" in err()
    assert c(form, orders=u32(3, 0, 0)) == INVALID and b"unknown order class" in err()
    assert c(form, kinds=u32(1, 16, 32), orders=u32(2, 0, 0)) == INVALID and b"width of 4 or 8" in err()
    assert c(form, nrows=(1 << 32) - 1) == INVALID and b"2^32 - 2" in err()
    assert c(form, offsets=ptrs(None, None, None)) == INVALID and b"without offsets" in err()
    assert c(form, values=ptrs(None, c.bools, c.text)) == INVALID and b"has no values" in err()
    if form == "host":   # the host form reads the offsets: the device form's are on the device
        assert c(form, offsets=ptrs(None, None, (ctypes.c_int32 * 4)(1, 3, 2, 6))) == INVALID and b"decrease" in err()
        assert c(form, offsets=ptrs(None, None, (ctypes.c_int32 * 4)(-1, 3, 3, 6))) == INVALID and b"negative" in err()
        assert c(form, values=ptrs(c.ints, c.bools, None)) == INVALID and b"bytes but no values" in err()
    assert c(form, stats=None) == INVALID and b"stats4 is NULL" in err()
    # the order of the checks
    assert c(form, kinds=None, nkeys=0) == INVALID and b"is NULL" in err()
    assert c(form, nkeys=0, kinds=u32(4, 33, 32)) == INVALID and b"nkeys is 0" in err()
    assert c(form, kinds=u32(1, 33, 32), orders=u32(2, 0, 0)) == INVALID and b"unknown kind" in err()
    assert c(form, kinds=u32(1, 16, 32), orders=u32(2, 0, 0), nrows=1 << 33) == INVALID and b"width of 4 or 8" in err()
    assert c(form, nrows=1 << 33, stats=None) == INVALID and b"2^32 - 2" in err()
    assert c(form, offsets=ptrs(None, None, None), stats=None) == INVALID and b"without offsets" in err()
    assert c.untouched()
    # well formed: past every check above, to the device question -- with every combination of NULL outputs
    assert past_the_argument_checks(c(form))
    for mask in range(16):
        assert past_the_argument_checks(c(form, outs=[None if mask >> k & 1 else o for k, o in enumerate(c.outs)])), mask
    assert past_the_argument_checks(c(form, orders=u32(2, 77, 99)))                     # ignored for booleans and bytes
    if form == "device":   # the most rows there may be (the host form would read that many offsets)
        assert past_the_argument_checks(c(form, nrows=(1 << 32) - 2))
    assert c.untouched()


def test_no_rows_is_ok_without_a_device(built_lib):
    c = Call()
    for form in FORMS:
        for k in range(4):
            c.stats[k] = 7
        assert c(form, nrows=0) == OK and list(c.stats) == [0, 0, 0, 0] and all(list(o) == [9, 9, 9] for o in c.outs)
        assert c(form, nrows=0, outs=[None] * 4, values=ptrs(None, None, None), offsets=ptrs(None, None, None)) == OK
        assert c(form, nrows=0, nkeys=0) == INVALID              # ... after the argument checks
        assert c(form, nrows=0, stats=None) == INVALID
    import torch

    if not torch.cuda.is_available():
        g = tabular.group_rows([np.zeros(0, dtype=np.int64)])
        assert all(a.size == 0 and a.dtype == np.uint32 for a in g[:4]) and g.stats == (0, 0, 0, 0)


def test_no_cpu_path_for_the_grouping(built_lib):
    import torch

    c = Call()
    for form in FORMS:
        assert past_the_argument_checks(c(form))
    assert c.untouched()
    if not torch.cuda.is_available():   # the Python layer hands the status on
        for call in (lambda: tabular.group_rows([np.arange(4, dtype=np.int64)]),
                     lambda: tabular.unique({"a": np.arange(4, dtype=np.int64)}, "a"),
                     lambda: tabular.n_duped_rows({"a": np.arange(4, dtype=np.int64)}, ["a"])):
            with pytest.raises(_capi.OxenError) as e:
                call()
            assert e.value.code == NODEVICE, e.value
    # the orders default as the sort's do: raw uint8 storage does not say whether it holds floats
    raw = Column(8, 2, np.zeros(16, dtype=np.uint8))
    with pytest.raises(_capi.OxenError, match="sort key column 1") as e:
        tabular.group_rows([np.arange(2, dtype=np.int64), raw])
    assert e.value.code == INVALID
    with pytest.raises(_capi.OxenError, match="one entry per key"):
        tabular.group_rows([np.arange(2, dtype=np.int64)], orders=[0, 0])
    with pytest.raises(_capi.OxenError, match="not in the frame"):
        tabular.unique({"a": np.arange(2, dtype=np.int64)}, "ghost")
    with pytest.raises(_capi.OxenError, match="at least one key"):
        tabular.unique_count({"a": np.arange(2, dtype=np.int64)}, [])


def test_host_pieces_native_program(built_lib, tmp_path):
    """The argument checks, the lease's layout and the staging plan in a program of their own: as build.py
    builds it, and under -fsanitize=address,undefined. Nothing is loaded into python under a sanitizer."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.GROUP_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    exe = str(tmp_path / "group_rows_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.GROUP_TEST_SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---------------------------------------------------------------- the restatement
def test_restatement_on_small_cases():
    g = _grouprows.group_rows([column(np.array([5, 7, 5, 5, 9, 7], dtype=np.int64))])
    assert g.group.tolist() == [0, 1, 0, 0, 4, 1] and g.count.tolist() == [3, 2, 3, 3, 1, 2]
    assert g.first_idx.tolist() == [0, 1, 4] and g.first_count.tolist() == [3, 2, 1] and g.stats == (3, 5, 3, 0)
    # the pairs the row hashes cannot tell apart
    a, b = column(["ab", "a"]), column(["c", "bc"])
    assert _grouprows.group_rows([a, b]).stats[0] == 2
    x = column(np.array([0, 5], dtype=np.int64), validity=[False, True])
    y = column(np.array([5, 0], dtype=np.int64), validity=[True, False])
    assert _grouprows.group_rows([x, y]).stats[0] == 2
    assert _grouprows.group_rows([column([None, "", None, ""])]).group.tolist() == [0, 1, 0, 1]
    assert _grouprows.group_rows([column(np.array([0, 0], dtype=np.int64), validity=[False, True])]).stats[0] == 2
    f = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, 5e-324], dtype=np.float64)
    assert _grouprows.group_rows([column(f)], [_grouprows.FLOAT]).group.tolist() == [0, 0, 2, 2, 4, 5]
    assert _grouprows.group_rows([column(f)], [_grouprows.UNSIGNED]).stats[0] == 6
    # a 240-byte image is short, 241 long: tag + 4 bytes of length + the cell
    cells = [b"x" * 235, b"x" * 236, b"x" * 235]
    assert _grouprows.group_rows([_grouprows.strings(cells)]).stats == (2, 2, 2, 1)
    assert _grouprows.group_rows([_grouprows.strings(cells, _grouprows.BYTES64)]).stats == (2, 2, 2, 3)


def golden_frame(case, dtypes, which="frame"):
    """A frame of the fixture as {name: Column}; `count` is UInt32, as polars' len() is."""
    numpy_of = {"f64": np.float64, "bool": bool}
    out = {}
    for name, values in case[which].items():
        dt = dtypes[name]
        if dt == "str":
            out[name] = column(values)
        elif dt == "u32":
            out[name] = Column(4, len(values), np.array(values, dtype=np.uint32))
        else:
            out[name] = column(np.array(values, dtype=numpy_of[dt]))
    return out


def restated(case, dtypes):
    """The case's operation by the restatements: the grouping, the take through first_idx, the sort."""
    frame = golden_frame(case, dtypes)
    keys = [frame[name] for name in case["fields"]]
    g = _grouprows.group_rows(keys)
    names = list(frame) if case["op"] == "unique" else case["fields"]
    taken = _take.take([frame[name] for name in names], g.first_idx)
    out = {name: Column(t.kind, t.nrows, t.values, t.offsets, t.validity) for name, t in zip(names, taken)}
    if case["op"] == "unique_count":
        out["count"] = Column(4, g.first_count.size, g.first_count)
    perm, _ = _sortrows.sort_indices([out[case["sort_by"]]])
    taken = _take.take(list(out.values()), perm)
    return {name: _take.pylist(Column(t.kind, t.nrows, t.values, t.offsets, t.validity)) for name, t in zip(out, taken)}, g


def test_restatement_reproduces_the_reference_s_recorded_frames():
    """The three unit tests of the reference (tabular.rs:1803-1901): `unique` on label, on image,label, then
    sort_by image; `unique_count` on label then sort_by label, which gives dog 3 and unknown 1."""
    fx = json.load(open(GOLDEN))
    assert [c["name"] for c in fx["cases"]] == ["test_unique_single_field", "test_unique_multi_field", "test_unique_count_single_field"]
    for case in fx["cases"]:
        got, g = restated(case, fx["dtypes"])
        want = golden_frame(case, fx["dtypes"], "expected")
        assert list(got) == list(want), case["name"]
        for name, c in want.items():
            assert got[name] == _take.pylist(c), (case["name"], name)
    assert restated(fx["cases"][2], fx["dtypes"])[1].stats == (2, 3, 3, 0)
    assert restated(fx["cases"][0], fx["dtypes"])[1].first_idx.tolist() == [0, 2]


def fake_group_rows(columns, orders=None, ctx=None):
    cols = tabular._as_columns(columns)
    g = _grouprows.group_rows(cols, list(tabular._orders(cols, orders)))
    return RowGroups(g.group, g.count, g.first_idx, g.first_count, GroupStats(*g.stats))


def fake_take(columns, idx0, idx1=None, plan=None, ctx=None):
    entries = plan if plan is not None else [(k, 0, None, 0) for k in range(len(columns))]
    out = []
    for entry, t in zip(entries, _take.take(columns, idx0, idx1, plan)):
        src = columns[entry[0]].values
        values = t.values.view(src.dtype) if t.kind in (1, 4, 8) and src.dtype.itemsize == t.kind else t.values
        out.append(Column(t.kind, t.nrows, values, t.offsets, t.validity))
    return out


def test_compositions_over_the_restatements(monkeypatch):
    """`unique`, `unique_count`, `is_duplicated` and `n_duped_rows` with `group_rows` and `take` answered by the
    restatements: which columns are keys, which are taken, the count column's kind."""
    monkeypatch.setattr(tabular, "group_rows", fake_group_rows)
    monkeypatch.setattr(tabular, "take", fake_take)
    fx = json.load(open(GOLDEN))
    frame = golden_frame(fx["cases"][2], fx["dtypes"])
    counted = tabular.unique_count(frame, "label")
    assert list(counted) == ["label", "count"] and _take.pylist(counted["label"]) == ["dog", "unknown"]
    assert counted["count"].kind == _capi.OXH_COL_FIXED4 and counted["count"].values.dtype == np.uint32
    assert counted["count"].values.tolist() == [3, 1] and counted["count"].nrows == 2
    assert tabular.is_duplicated(frame, ["label"]).tolist() == [True, True, False, True]
    assert tabular.n_duped_rows(frame, ["label"]) == 3 and tabular.n_duped_rows(frame, ["image", "label"]) == 0
    u = tabular.unique(golden_frame(fx["cases"][1], fx["dtypes"]), ["image", "label"])
    assert list(u) == ["image", "label", "min_x", "max_x", "is_correct"] and _take.pylist(u["min_x"]) == _take.pylist(column(np.array([0.0, 2.0])))
    f = {"x": column(np.array([0.0, -0.0, 1.0], dtype=np.float64))}
    assert tabular.n_duped_rows(f, "x") == 2 and tabular.n_duped_rows(f, "x", orders=[_capi.OXH_SORT_UNSIGNED]) == 0
    assert tabular.n_duped_rows(f, "x", orders={"x": _capi.OXH_SORT_UNSIGNED}) == 0
