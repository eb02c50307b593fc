"""Chunk overlap between file versions (oxh_chunk_overlap_*, oxen_amd.dedup.chunk_overlap / OxenChunker)
without a GPU: the ABI is declared, exported and bound; every argument error comes back without a
device; there is no CPU path (OXH_ERR_NODEVICE); the host-only pieces of the Python mirror."""
import ctypes
import subprocess

import numpy as np
import pytest

from oxen_amd import _capi, dedup

FUNCTIONS = ["oxh_chunk_overlap_device", "oxh_chunk_overlap_host"]
U64P = _capi._u64p


def u64(*values):
    return (ctypes.c_uint64 * len(values))(*values)


def test_the_two_functions_are_declared_exported_and_bound(built_lib):
    assert set(FUNCTIONS) <= set(_capi.header_symbols())
    assert set(FUNCTIONS) <= set(_capi.SIGNATURES)
    assert not [s for s in FUNCTIONS if "dedup_index" in s]
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(FUNCTIONS) <= exported
    L = _capi.lib()
    vp, u, p = ctypes.c_void_p, ctypes.c_uint64, U64P
    # int f(oxh_ctx*, const uint64_t* d_digests, const uint64_t* d_lens, const uint64_t* set_first,
    #       uint64_t nsets, uint64_t* rows_out, uint64_t* bytes_out[, void* stream]): device pointers are void*
    assert L.oxh_chunk_overlap_device.argtypes == [vp, vp, vp, p, u, p, p, vp]
    assert L.oxh_chunk_overlap_host.argtypes == [vp, p, p, p, u, p, p]
    for name in FUNCTIONS:
        assert getattr(L, name).argtypes == _capi.SIGNATURES[name][1]
        assert getattr(L, name).restype == ctypes.c_int
    assert L.oxh_abi_version() == 5  # additive: the version stays
    hdr = open(_capi.HEADER).read()
    assert "#define OXH_CHUNK_OVERLAP_MAX_SETS 256" in hdr and dedup.OXH_CHUNK_OVERLAP_MAX_SETS == 256


def host(ctx, digests, lens, set_first, nsets, rows_out, bytes_out):
    return _capi.lib().oxh_chunk_overlap_host(ctx, digests, lens, set_first, nsets, rows_out, bytes_out)


def device(ctx, digests, lens, set_first, nsets, rows_out, bytes_out):
    return _capi.lib().oxh_chunk_overlap_device(ctx, ctypes.cast(digests, ctypes.c_void_p) if digests else None,
                                                ctypes.cast(lens, ctypes.c_void_p) if lens else None, set_first, nsets,
                                                rows_out, bytes_out, None)


@pytest.mark.parametrize("call", [host, device], ids=["host", "device"])
def test_argument_errors_need_no_device(built_lib, call):
    """Each of these is OXH_ERR_INVALID whether or not a device is there, with a NULL context: the
    argument checks come before OXH_ERR_NODEVICE and before the context is looked at."""
    INVALID = _capi.OXH_ERR_INVALID
    dig, lens = u64(*range(12)), u64(*range(6))
    rows, nbytes = u64(*[7] * 9), u64(*[7] * 9)
    first = u64(0, 2, 4, 6)
    assert call(None, dig, lens, None, 3, rows, nbytes) == INVALID          # NULL set_first
    assert call(None, dig, lens, first, 3, None, nbytes) == INVALID         # NULL rows_out
    assert call(None, dig, lens, first, 0, rows, nbytes) == INVALID         # nsets == 0
    big = u64(*range(258))
    many = u64(*[0] * (257 * 257))
    assert call(None, u64(*range(2 * 257)), None, big, 257, many, None) == INVALID   # nsets > 256
    assert call(None, dig, lens, u64(1, 2, 4, 6), 3, rows, nbytes) == INVALID       # set_first[0] != 0
    assert call(None, dig, lens, u64(0, 4, 2, 6), 3, rows, nbytes) == INVALID       # a decreasing set_first
    assert call(None, None, None, first, 3, rows, None) == INVALID                  # NULL digests with N > 0
    assert call(None, dig, None, u64(0, 2, 4, (1 << 40) + 1), 3, rows, None) == INVALID  # N > 2^40
    assert call(None, dig, None, first, 3, rows, nbytes) == INVALID                 # bytes_out without lengths
    assert list(rows) == [7] * 9 and list(nbytes) == [7] * 9                        # outputs untouched
    assert b"chunk overlap" in _capi.lib().oxh_last_error()


def test_no_overlap_without_a_device(built_lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("the no-device branch needs a host without a GPU")
    NODEVICE = _capi.OXH_ERR_NODEVICE
    dig, lens, rows, nbytes = u64(*range(12)), u64(*range(6)), u64(*[7] * 9), u64(*[7] * 9)
    for call in (host, device):
        assert call(None, dig, lens, u64(0, 2, 4, 6), 3, rows, nbytes) == NODEVICE   # before the NULL context
        assert call(None, dig, None, u64(0, 2, 4, 6), 3, rows, None) == NODEVICE
        assert call(None, None, None, u64(0, 0), 1, rows, None) == NODEVICE          # N == 0 comes after it too
    assert list(rows) == [7] * 9
    sets = [np.array([(1, 2), (3, 4)], dtype=np.uint64), np.array([(1, 2)], dtype=np.uint64)]
    with pytest.raises(_capi.OxenError) as e:
        dedup.chunk_overlap(sets)
    assert e.value.code == NODEVICE, e.value
    with pytest.raises(_capi.OxenError) as e:
        dedup.count_commit_overlap(["1", "2"], ["2"])
    assert e.value.code == NODEVICE, e.value


def test_chunk_overlap_checks_shapes_before_any_call():
    with pytest.raises(_capi.OxenError) as e:
        dedup.chunk_overlap([np.zeros((3, 3), dtype=np.uint64)])
    assert e.value.code == _capi.OXH_ERR_INVALID
    with pytest.raises(_capi.OxenError) as e:
        dedup.chunk_overlap([np.zeros((3, 2), dtype=np.uint64)], lens=[np.zeros(2, dtype=np.uint64)])
    assert e.value.code == _capi.OXH_ERR_INVALID


def test_names_to_digests_is_the_inverse_of_chunk_name():
    ones = (1 << 64) - 1
    values = [0, 1, ones, 1 << 64, (1 << 64) + 5, (1 << 128) - 1, 0x0123456789ABCDEF_FEDCBA9876543210]
    names = [str(v) for v in values]
    rows = dedup.names_to_digests(names)
    assert rows.dtype == np.uint64 and rows.shape == (len(values), 2)
    assert rows.tolist() == [[v & ones, v >> 64] for v in values]
    assert [dedup.chunk_name(lo, hi) for lo, hi in rows.tolist()] == names
    for lo, hi in [(0, 0), (ones, 0), (0, 1), (ones, ones), (12345, 67890)]:
        assert dedup.names_to_digests([dedup.chunk_name(lo, hi)]).tolist() == [[lo, hi]]
    assert dedup.names_to_digests([]).shape == (0, 2)
    for bad in (str(1 << 128), "-1", "0x10", "007"):
        with pytest.raises((_capi.OxenError, ValueError)):
            dedup.names_to_digests([bad])


def test_version_path(tmp_path):
    c = dedup.OxenChunker(8192, "fastcdc", str(tmp_path / "versions" / "files"))
    h = "a1b2c3d4e5f60718293a4b5c6d7e8f90"
    root = str(tmp_path / "versions" / "files")
    assert c.version_dir(h) == f"{root}/a1/b2c3d4e5f60718293a4b5c6d7e8f90"
    assert c.version_path(h) == f"{root}/a1/b2c3d4e5f60718293a4b5c6d7e8f90/data"
    assert (c.chunk_size, c.chunk_algorithm, c.root_path) == (8192, "fastcdc", root)


def test_rust_debug_text_of_a_string_vector():
    assert dedup.rust_debug_strings([]) == "[]"
    assert dedup.rust_debug_strings(["1"]) == '["1"]'
    assert dedup.rust_debug_strings(["1", "22", "340282366920938463463374607431768211455"]) == \
        '["1", "22", "340282366920938463463374607431768211455"]'


def test_pack_without_commits_raises(tmp_path):
    c = dedup.OxenChunker(8192, "fastcdc", str(tmp_path))
    with pytest.raises(ValueError):
        c.pack("fastcdc", 8192, [], str(tmp_path / "out"))
    with pytest.raises(ValueError):
        c.pack("fastcdc", 8192, [("c0", None)], str(tmp_path / "out"), n=0)


def test_unpack_is_the_reference_stub(tmp_path, capsys):
    c = dedup.OxenChunker(8192, "fastcdc", str(tmp_path))
    assert c.unpack(str(tmp_path / "in"), str(tmp_path / "out.bin")) == str(tmp_path / "out.bin")
    assert "Unpacking repository data" in capsys.readouterr().out and not (tmp_path / "out.bin").exists()


def test_reexported_from_the_package():
    import oxen_amd

    for name in ("ChunkOverlap", "chunk_overlap", "chunk_overlap_device", "names_to_digests", "count_commit_overlap",
                 "OxenChunker"):
        assert getattr(oxen_amd, name) is getattr(dedup, name)
