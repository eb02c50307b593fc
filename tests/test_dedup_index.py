"""The dedup index (oxh_dedup_index_*, oxen_amd.dedup.DedupIndex / dedup_report) without a GPU: the
ABI is declared, exported and bound; there is no CPU index (OXH_ERR_NODEVICE); the report's arithmetic
over a stub index that answers with the dict loop the GPU tests compare against."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi, dedup

FUNCTIONS = ["oxh_dedup_index_create", "oxh_dedup_index_destroy", "oxh_dedup_index_insert_device",
             "oxh_dedup_index_insert_host", "oxh_dedup_index_query_device", "oxh_dedup_index_query_host",
             "oxh_dedup_index_counts"]


class StubIndex:
    """What a DedupIndex answers, as a dict loop: first[i] = seen.setdefault(key, ordinal)."""

    def __init__(self):
        self.seen, self.rows, self.life = {}, 0, [0, 0, 0, 0]

    def counts(self):
        return dedup.DedupCounts(*self.life)

    def insert(self, digests, lens=None):
        first, s = [], [0, 0, 0, 0]
        for i, key in enumerate(map(tuple, np.asarray(digests, dtype=np.uint64).reshape(-1, 2).tolist())):
            r = self.rows + i
            first.append(self.seen.setdefault(key, r))
            ln = int(lens[i]) if lens is not None else 0
            new = first[-1] == r
            s[0 if new else 2] += 1
            s[1 if new else 3] += ln
        self.rows += len(first)
        for k, v in enumerate((s[0] + s[2], s[0], s[1] + s[3], s[1])):
            self.life[k] += v
        return np.array(first, dtype=np.uint64), dedup.DedupStats(*s)


def test_the_seven_functions_are_declared_exported_and_bound(built_lib):
    assert set(FUNCTIONS) <= set(_capi.header_symbols())
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    assert [s for s in _capi.header_symbols() if "dedup_index" in s] == sorted(FUNCTIONS)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    L = _capi.lib()
    for name in FUNCTIONS:
        assert getattr(L, name).argtypes == _capi.SIGNATURES[name][1]
    assert L.oxh_abi_version() == 5  # additive: the version stays


def test_the_handle_is_a_plain_void_pointer():
    """A fifth opaque struct would need a new Rust type; the handle is `void*` as `stream` is."""
    hdr = open(_capi.HEADER).read()
    assert re.search(r"int oxh_dedup_index_create\(oxh_ctx\* ctx, uint64_t capacity_rows, void\*\* out\);", hdr)
    assert not re.search(r"typedef struct oxh_dedup", hdr)


def test_argument_errors_need_no_device(built_lib):
    L = _capi.lib()
    assert L.oxh_dedup_index_create(None, 0, None) == _capi.OXH_ERR_INVALID
    assert L.oxh_dedup_index_destroy(None) == _capi.OXH_OK
    four = (ctypes.c_uint64 * 4)()
    assert L.oxh_dedup_index_counts(None, four) == _capi.OXH_ERR_INVALID
    assert L.oxh_dedup_index_insert_host(None, None, None, 0, None, None) == _capi.OXH_ERR_INVALID
    assert L.oxh_dedup_index_query_host(None, None, 0, None) == _capi.OXH_ERR_INVALID


def test_no_index_without_a_device(built_lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("the no-device branch needs a host without a GPU")
    with pytest.raises(_capi.OxenError) as e:
        dedup.DedupIndex()
    assert e.value.code == _capi.OXH_ERR_NODEVICE, e.value
    h = ctypes.c_void_p()
    assert _capi.lib().oxh_dedup_index_create(None, 0, ctypes.byref(h)) == _capi.OXH_ERR_NODEVICE
    assert not h.value
    with pytest.raises(_capi.OxenError):
        dedup.dedup_report(dedup.FastCdcTable(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64),
                                              np.zeros(1, np.uint64)))


def _row(chunks, distinct, nbytes, distinct_bytes):
    return {"chunks": chunks, "distinct_chunks": distinct, "bytes": nbytes, "distinct_bytes": distinct_bytes,
            "ratio": distinct_bytes / nbytes if nbytes else 1.0}


def test_report_arithmetic_fastcdc_table():
    # three files: a b a | (empty) | b c c, lengths by row
    a, b, c = (1, 10), (1, 11), (2, 10)  # a and b share lo, a and c share hi
    dig = np.array([a, b, a, b, c, c], dtype=np.uint64)
    lens = np.array([100, 200, 100, 200, 50, 50], dtype=np.uint64)
    tab = dedup.FastCdcTable(np.zeros(6, np.uint64), lens, dig, np.array([0, 3, 3, 6], dtype=np.uint64))
    rep = dedup.dedup_report(tab, StubIndex())
    assert rep["files"] == [_row(3, 2, 400, 300), _row(0, 0, 0, 0), _row(3, 1, 300, 50)]
    del rep["files"]
    assert rep == _row(6, 3, 700, 350) and rep["ratio"] == 0.5


def test_report_counts_against_what_the_index_already_holds():
    idx = StubIndex()
    idx.insert(np.array([(7, 7), (1, 11)], dtype=np.uint64), np.array([9, 200], dtype=np.uint64))
    dig = np.array([(1, 10), (1, 11), (7, 7), (3, 3)], dtype=np.uint64)
    tab = dedup.FastCdcTable(np.zeros(4, np.uint64), np.array([100, 200, 9, 1], dtype=np.uint64), dig,
                             np.array([0, 4], dtype=np.uint64))
    rep = dedup.dedup_report(tab, idx)
    assert rep["files"] == [_row(4, 2, 310, 101)]
    assert idx.counts() == dedup.DedupCounts(6, 4, 519, 310)


def test_report_derives_fixed_size_lengths():
    # 4 KiB chunks: 10 000 B -> 4096 4096 1808; 4096 B -> 4096; 0 B -> none; 1 B -> 1
    sizes = np.array([10_000, 4096, 0, 1], dtype=np.uint64)
    first = np.array([0, 3, 4, 4, 5], dtype=np.uint64)
    dig = np.array([(5, 5), (5, 5), (6, 6), (5, 5), (8, 8)], dtype=np.uint64)
    tab = dedup.FixedChunkTable(dig, first, sizes, chunk_size=4096)
    assert dedup.table_lens(tab).tolist() == [4096, 4096, 1808, 4096, 1]
    rep = dedup.dedup_report(tab, StubIndex())
    assert rep["files"] == [_row(3, 2, 10_000, 5904), _row(1, 0, 4096, 0), _row(0, 0, 0, 0), _row(1, 1, 1, 1)]
    assert (rep["chunks"], rep["distinct_chunks"], rep["bytes"], rep["distinct_bytes"]) == (5, 3, 14_097, 5905)
    # the chunk size may also be given by the caller; without one, or with a wrong one, it is an error
    bare = dedup.FixedChunkTable(dig, first, sizes)
    assert dedup.table_lens(bare, 4096).tolist() == [4096, 4096, 1808, 4096, 1]
    with pytest.raises(_capi.OxenError):
        dedup.table_lens(bare)
    with pytest.raises(_capi.OxenError):
        dedup.table_lens(bare, 8192)


def test_insert_rejects_misshapen_digests_before_any_call():
    idx = dedup.DedupIndex.__new__(dedup.DedupIndex)
    idx.handle = ctypes.c_void_p(1)  # never reaches the library: the shape check comes first
    try:
        with pytest.raises(_capi.OxenError):
            idx.insert(np.zeros((3, 3), dtype=np.uint64))
        with pytest.raises(_capi.OxenError):
            idx.insert(np.zeros((3, 2), dtype=np.uint64), lens=np.zeros(2, dtype=np.uint64))
    finally:
        idx.handle = None
