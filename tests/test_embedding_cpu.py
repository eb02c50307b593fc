"""The embedding query (oxh_embedding_*, oxen_amd.tabular) without a GPU: the six entries are declared, exported and
bound at ABI version 5; every argument error comes back as OXH_ERR_INVALID, in the header's order, before
OXH_ERR_NODEVICE, and there is no CPU path; the host forms validate offsets and indices before anything is
copied; the order key, the page arithmetic, the mean's partition and the staging plan in a program of their own
(embedding_host.hpp, the code the kernels and the entries run); the restatement of tests/_embedding.py pinned to
a hand-computed fixture (tests/golden/embedding.json); `embedding_from_arrow` on sliced, chunked and nullable
pyarrow arrays."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _embedding as E
from oxen_amd import _capi, tabular
from oxen_amd.tabular import Embedding

FUNCTIONS = ["oxh_embedding_mean_device", "oxh_embedding_mean_host", "oxh_embedding_similarity_device",
             "oxh_embedding_similarity_host", "oxh_embedding_take_device", "oxh_embedding_take_host"]
INVALID, NODEVICE, OK = _capi.OXH_ERR_INVALID, _capi.OXH_ERR_NODEVICE, _capi.OXH_OK
VP = ctypes.c_void_p
FORMS = ["host", "device"]
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embedding.json")))


def err():
    return _capi.lib().oxh_last_error()


def test_the_six_functions_are_declared_exported_and_bound(built_lib):
    assert [s for s in _capi.header_symbols() if "embedding" in s] == FUNCTIONS
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    assert _capi.lib().oxh_abi_version() == 5  # additive: the version stays
    assert [len(_capi.SIGNATURES[f][1]) for f in FUNCTIONS] == [13, 12, 15, 14, 14, 13]
    header = open(_capi.HEADER).read()
    for name in ("OXH_EMB_FIXED", "OXH_EMB_LIST32", "OXH_EMB_LIST64"):
        assert f"#define {name} {getattr(_capi, name)}" in header, name
    assert (_capi.OXH_EMB_FIXED, _capi.OXH_EMB_LIST32, _capi.OXH_EMB_LIST64) == (E.FIXED, E.LIST32, E.LIST64)
    assert E.TAKE_NULL == _capi.OXH_TAKE_NULL
    assert "NOT pinned by a run of DuckDB" in header
    import oxen_amd

    for name in ("Embedding", "EmbeddingStats", "Similarity", "embedding", "embedding_from_arrow", "embedding_to_arrow", "embedding_mean",
                 "embedding_mean_device", "cosine_similarity", "cosine_similarity_device", "embedding_take", "embedding_take_device",
                 "page_rows", "nearest_neighbors", "nearest_neighbors_device", "sort_by_similarity", "sort_by_similarity_device"):
        assert getattr(oxen_amd, name) is getattr(tabular, name), name
    assert Embedding._fields == ("layout", "dim", "nrows", "values", "offsets", "validity", "validity_bit")
    assert tabular.Similarity._fields == ("sim", "validity", "order_key", "perm", "stats")
    assert tabular.EmbeddingStats._fields == ("used", "null_rows", "wrong_length", "first_wrong")


class Call:
    """Well-formed calls as the raw ABI takes them: a List<float32> column of 3 rows of dim 2 whose first offset is
    not 0, with a validity bitmap. The outputs hold sentinels."""

    def __init__(self):
        self.values = (ctypes.c_float * 8)(9, 1, 0, 0, 1, 1, 1, 9)
        self.off = (ctypes.c_int32 * 4)(1, 3, 5, 7)
        self.valid = (ctypes.c_uint8 * 1)(0b111)
        self.query = (ctypes.c_float * 2)(1, 0)
        self.idx = (ctypes.c_uint32 * 2)(0, 2)
        self.out = (ctypes.c_float * 4)(7, 7, 7, 7)
        self.sim = (ctypes.c_float * 3)(7, 7, 7)
        self.bitmap = (ctypes.c_uint8 * 1)(0xA5)
        self.key = (ctypes.c_uint32 * 3)(9, 9, 9)
        self.perm = (ctypes.c_uint32 * 3)(9, 9, 9)
        self.stats = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        self.col = dict(layout=1, nrows=3, dim=2, values=self.values, offsets=self.off, validity=self.valid, bit=0)
        self.own = {"mean": dict(idx=self.idx, n=2, out=self.out, stats=self.stats),
                    "similarity": dict(query=self.query, sim=self.sim, sim_validity=self.bitmap, key=self.key, perm=self.perm, stats=self.stats),
                    "take": dict(idx=self.idx, n=2, out=self.out, out_validity=self.bitmap, stats=self.stats)}

    def untouched(self):
        return (list(self.out) == [7] * 4 and list(self.sim) == [7] * 3 and list(self.bitmap) == [0xA5] and list(self.key) == [9] * 3
                and list(self.perm) == [9] * 3 and list(self.stats) == [7] * 4)

    def __call__(self, entry, form, **change):
        a = {**self.col, **self.own[entry], **change}
        cast = lambda x: ctypes.cast(x, VP) if x is not None and not isinstance(x, int) else x  # noqa: E731
        args = [None, a["layout"], a["nrows"], a["dim"], cast(a["values"]), cast(a["offsets"]), cast(a["validity"]), a["bit"]]
        if entry == "mean":
            args += [cast(a["idx"]), a["n"], cast(a["out"]), a["stats"]]
        elif entry == "similarity":
            args += [cast(a["query"]), cast(a["sim"]), cast(a["sim_validity"]), cast(a["key"]), cast(a["perm"]), a["stats"]]
        else:
            args += [cast(a["idx"]), a["n"], cast(a["out"]), cast(a["out_validity"]), a["stats"]]
        fn = getattr(_capi.lib(), f"oxh_embedding_{entry}_{form}")
        return fn(*args) if form == "host" else fn(*args, None)


def past_the_argument_checks(rc):
    """What a well-formed call with a NULL context gives: OXH_ERR_NODEVICE where there is no device, and the
    NULL context's own OXH_ERR_INVALID where there is one."""
    import torch

    if not torch.cuda.is_available():
        return rc == NODEVICE
    return rc == INVALID and b"ctx is NULL" in err()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("entry", ["mean", "similarity", "take"])
def test_embedding_argument_errors_need_no_device(built_lib, entry, form):
    """Each of these is OXH_ERR_INVALID whether or not a device is there, with a NULL context; the order of the
    checks is the header's: the column, the entry's own arguments, stats4, the host form's indices, the context."""
    c = Call()
    name = f"embedding {entry}".encode()
    assert c(entry, form, layout=3) == INVALID and b"unknown layout" in err() and name in err()          # 1. the column
    assert c(entry, form, layout=3, dim=0) == INVALID and b"unknown layout" in err()
    assert c(entry, form, dim=0) == INVALID and b"dim is 0" in err()
    assert c(entry, form, dim=0, nrows=(1 << 32) - 1) == INVALID and b"dim is 0" in err()
    assert c(entry, form, nrows=(1 << 32) - 1) == INVALID and b"2^32 - 2" in err()
    assert c(entry, form, values=ctypes.addressof(c.values) + 2) == INVALID and b"4-byte aligned" in err()
    assert c(entry, form, offsets=None) == INVALID and b"without offsets" in err()
    assert c(entry, form, layout=0, offsets=None, values=None) == INVALID and b"no values" in err()
    if form == "host":   # the host forms read the offsets: the device forms' are on the device
        assert c(entry, form, offsets=(ctypes.c_int32 * 4)(1, 3, 2, 7)) == INVALID and b"decrease at row 1" in err()
        assert c(entry, form, offsets=(ctypes.c_int32 * 4)(-1, 3, 5, 7)) == INVALID and b"negative" in err()
        assert c(entry, form, values=None) == INVALID and b"elements but no values" in err()
    if entry == "mean":                                                                                   # 2. its own
        assert c(entry, form, n=(1 << 32) - 1) == INVALID and b"indices" in err()
        assert c(entry, form, idx=None) == INVALID and b"idx is NULL" in err()
        assert c(entry, form, out=None) == INVALID and b"out is NULL" in err()
        assert c(entry, form, out=None, stats=None) == INVALID and b"out is NULL" in err()
    elif entry == "similarity":
        assert c(entry, form, key=None) == INVALID and b"perm needs order_key" in err()
        assert c(entry, form, query=None) == INVALID and b"query is NULL" in err()
        assert c(entry, form, sim=None) == INVALID and b"sim is NULL" in err()
        assert c(entry, form, sim_validity=None) == INVALID and b"sim_validity is NULL" in err()
        assert c(entry, form, sim_validity=None, stats=None) == INVALID and b"sim_validity is NULL" in err()
    else:
        assert c(entry, form, n=(1 << 32) - 1) == INVALID and b"output rows" in err()
        for table in ("idx", "out", "out_validity"):
            assert c(entry, form, **{table: None}) == INVALID and b"is NULL" in err(), table
    assert c(entry, form, stats=None) == INVALID and b"stats4 is NULL" in err()                           # 3.
    if form == "host" and entry != "similarity":                                                          # 4.
        assert c(entry, form, idx=(ctypes.c_uint32 * 2)(0, 3)) == INVALID and b"idx[1] = 3" in err()
        assert c(entry, form, idx=(ctypes.c_uint32 * 2)(0, 3), stats=None) == INVALID and b"stats4 is NULL" in err()
    assert c.untouched()
    assert past_the_argument_checks(c(entry, form))                                                      # 5. then the device / context
    # no rows (the take: no output rows) after the checks is OXH_OK with stats4 zeroed, GPU or not
    empty = dict(n=0) if entry == "take" else dict(nrows=0, values=None, offsets=None, validity=None)
    assert c(entry, form, **empty) == OK and list(c.stats) == [0, 0, 0, 0]
    c.stats[:] = [7, 7, 7, 7]
    assert c.untouched()
    assert c(entry, form, layout=3, **empty) == INVALID   # but the checks come first


def test_native_host_test_program(built_lib):
    """tests/native/embedding_host_test.cpp: the order key on hand-worked floats (strictly monotone, the null key
    unreachable), the argument checks, the offset validation, the mean's partition, the page arithmetic and the
    staging plan -- embedding_host.hpp, compiled without HIP."""
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.EMBEDDING_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def to_f32(v):
    return np.float32(float(v)) if isinstance(v, str) else np.float32(v)


def test_restatement_against_the_hand_computed_fixture():
    for case in GOLDEN["cosine"]:
        got, want = E.cosine(np.array(case["x"], np.float32), np.array(case["q"], np.float32)), to_f32(case["sim"])
        assert (math.isnan(got) and math.isnan(want)) or E.f32_bits(got) == E.f32_bits(want), case
        if "bits" in case:
            assert E.f32_bits(got) == int(case["bits"], 16)
        emb = tabular.embedding(np.array([case["x"]], np.float32))
        for ranked in (E.similarity(emb, case["q"]), E.similarity_exact(emb, case["q"])):   # the vectorised form agrees
            assert (math.isnan(got) and math.isnan(ranked.sim[0])) or ranked.sim.view(np.uint32)[0] == np.float32(got).view(np.uint32)
            assert ranked.stats == (1, 0, 0, 1) and ranked.key[0] == E.order_key(got)
    for case in GOLDEN["order_keys"]:
        assert E.order_key(int(case["sim_bits"], 16)) == int(case["key"], 16), case
    assert max(E.order_key(b) for b in range(0, 1 << 32, 0x10001)) <= 0xFF800000 < E.NULL_KEY
    sims = GOLDEN["ranking"]["sim"]
    keys = [E.NULL_KEY if s is None else E.order_key(to_f32(s)) for s in sims]
    assert E.stable_order(keys).tolist() == GOLDEN["ranking"]["perm"]
    m = GOLDEN["mean"]
    valid = [r is not None for r in m["rows"]]
    emb = tabular.embedding(np.array([r or [0, 0] for r in m["rows"]], np.float32), valid)
    for case in m["cases"]:
        got, stats = E.mean(emb, case["idx"])
        assert stats == tuple(case["stats"]), case
        assert (got is None) == (case["mean"] is None) and (got is None or got.tolist() == case["mean"]), case
    for p in GOLDEN["pages"]:
        assert E.page_rows(p["nrows"], p["size"], p["num"]) == (p["first"], p["count"]), p
        assert tabular.page_rows(p["nrows"], p["size"], p["num"]) == (p["first"], p["count"]), p
    with pytest.raises(_capi.OxenError):
        tabular.page_rows(10, -1, 1)


def test_restatement_of_the_three_layouts_and_the_take():
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, size=(6, 3)).astype(np.float32)
    valid = np.array([1, 0, 1, 1, 1, 1], bool)
    fixed = tabular.embedding(x, valid)
    off = np.array([2, 5, 8, 11, 14, 16, 19], np.int32)   # row 4 has two elements: a valid row of another length
    values = np.concatenate([np.full(2, 99, np.float32), x[:4].reshape(-1), x[4, :2], x[5]])
    listed = Embedding(E.LIST32, 3, 6, values, off, E.packed_at(valid, 3), 3)
    rows = E.rows(listed)
    assert rows[1] is None and rows[4] == E.WRONG and np.array_equal(rows[5], x[5]) and np.array_equal(rows[0], x[0])
    q = np.array([1, -2, 3], np.float32)
    a, b = E.similarity(fixed, q), E.similarity(listed, q)
    assert a.stats == (5, 1, 0, 6) and b.stats == (4, 1, 1, 4)
    keep = [0, 2, 3, 5]
    assert np.array_equal(a.sim.view(np.uint32)[keep], b.sim.view(np.uint32)[keep]) and b.sim[4] == 0 and b.key[4] == E.NULL_KEY
    assert a.validity.tolist() == [0b111101] and b.validity.tolist() == [0b101101]
    assert np.array_equal(E.similarity_exact(fixed, q).sim.view(np.uint32), a.sim.view(np.uint32))
    assert np.array_equal(E.similarity_exact(fixed, q).perm, a.perm) and np.array_equal(E.similarity_exact(fixed, q).key, a.key)
    got, validity, stats = E.take(listed, [5, E.TAKE_NULL, 1, 4, 0])
    assert validity.tolist() == [0b10001] and stats == (2, 2, 1, 4)
    assert np.array_equal(got.reshape(5, 3), np.stack([x[5], np.zeros(3), np.zeros(3), np.zeros(3), x[0]]).astype(np.float32))


# ---------------------------------------------------------------- pyarrow
def vectors_of(emb):
    return [None if v is None else (v if isinstance(v, str) else v.tolist()) for v in E.rows(emb)]


@pytest.mark.parametrize("kind", ["fixed", "list", "large_list"])
def test_embedding_from_arrow_sliced_chunked_and_nullable(kind):
    pa = pytest.importorskip("pyarrow")
    rows = [[1.0, 2.0, 3.0], None, [4.0, 5.0, 6.0], [7.0, 8.0, 9.0], None, [10.0, 11.0, 12.0], [13.0, 14.0, 15.0]]
    t = {"fixed": pa.list_(pa.float32(), 3), "list": pa.list_(pa.float32()), "large_list": pa.large_list(pa.float32())}[kind]
    whole = pa.array(rows, type=t)
    emb = tabular.embedding_from_arrow(whole)
    assert (emb.layout, emb.dim, emb.nrows) == ({"fixed": E.FIXED, "list": E.LIST32, "large_list": E.LIST64}[kind], 3, 7)
    assert vectors_of(emb) == rows
    assert emb.values.dtype == np.float32 and (emb.offsets is None) == (kind == "fixed")
    for lo, n in ((1, 5), (2, 3), (3, 0), (6, 1)):                      # slices keep their offsets: nothing is copied
        part = tabular.embedding_from_arrow(whole.slice(lo, n), dim=3)
        assert part.nrows == n and vectors_of(part) == rows[lo:lo + n], (lo, n)
        if n and kind != "fixed":
            assert int(part.offsets[0]) == sum(3 for r in rows[:lo] if r is not None)   # the first offset is not 0
    chunked = pa.chunked_array([whole.slice(0, 3), whole.slice(3, 4)])
    assert vectors_of(tabular.embedding_from_arrow(chunked)) == rows
    assert vectors_of(tabular.embedding_from_arrow(pa.chunked_array([whole.slice(2, 4)]))) == rows[2:6]
    no_nulls = tabular.embedding_from_arrow(pa.array([r for r in rows if r], type=t))
    assert no_nulls.validity is None and no_nulls.validity_bit == 0 and no_nulls.nrows == 5
    if kind != "fixed":
        # a child array with an offset of its own
        child = pa.array([99.0, 98.0] + [v for r in rows if r for v in r], type=pa.float32()).slice(2)
        offsets = pa.array([0, 3, 6, 9, 12, 15], type=pa.int64() if kind == "large_list" else pa.int32())
        made = (pa.LargeListArray if kind == "large_list" else pa.ListArray).from_arrays(offsets, child)
        assert vectors_of(tabular.embedding_from_arrow(made)) == [r for r in rows if r]
        ragged = pa.array([[1.0, 2.0, 3.0], [4.0, 5.0]], type=t)         # a row of another length is the calls' to refuse
        assert vectors_of(tabular.embedding_from_arrow(ragged)) == [[1.0, 2.0, 3.0], E.WRONG]
    back = tabular.embedding_to_arrow(tabular.embedding(np.arange(6, dtype=np.float32).reshape(2, 3), [True, False]))
    assert back.to_pylist() == [[0.0, 1.0, 2.0], None]


def test_embedding_from_arrow_refuses_what_the_reference_does():
    pa = pytest.importorskip("pyarrow")
    for bad in (pa.array([[1.0, 2.0]], type=pa.list_(pa.float64())), pa.array([[1.0, 2.0]], type=pa.list_(pa.float64(), 2)),
                pa.array([[1, 2]], type=pa.list_(pa.int32())), pa.array([1.0, 2.0], type=pa.float32()),
                pa.array([[1.0, None]], type=pa.list_(pa.float32())), pa.array([[1.0, None]], type=pa.list_(pa.float32(), 2)),
                pa.array([[1.0, None]], type=pa.large_list(pa.float32()))):
        with pytest.raises(_capi.OxenError) as e:
            tabular.embedding_from_arrow(bad)
        assert e.value.code == INVALID, bad.type
    # a null element outside the slice's span does not count
    some = pa.array([[1.0, None], [3.0, 4.0]], type=pa.list_(pa.float32()))
    assert vectors_of(tabular.embedding_from_arrow(some.slice(1, 1))) == [[3.0, 4.0]]
    with pytest.raises(_capi.OxenError):
        tabular.embedding(np.zeros(3, np.float32))
    with pytest.raises(_capi.OxenError):
        tabular.cosine_similarity(tabular.embedding(np.zeros((2, 3), np.float32)), [1.0, 2.0])
    frame = {"id": tabular.column(np.arange(3, dtype=np.int64))}
    with pytest.raises(_capi.OxenError):
        tabular.nearest_neighbors(frame, tabular.embedding(np.zeros((2, 3), np.float32)), [1.0, 2.0, 3.0], 10)
    with pytest.raises(_capi.OxenError) as e:   # an unknown field is an error before any device is needed
        tabular.sort_by_similarity(frame, tabular.embedding(np.zeros((3, 3), np.float32)), "nope == 1", 10)
    assert e.value.code == INVALID
