"""The batched Zstandard inflate on the GPU (oxh_zstd_inflate_*, oxen_amd/csrc/zstd_inflate.hip) against the plains the
fixtures were compressed from (tests/golden/make_zstd.py; the manifest's census says which forms each frame holds):
every fixture alone and all in one call, every malformed patch between two good frames, more frames than the grid, and
a frame without a content size through the list form."""
import zlib

import pytest

import _zstd_cases as Z
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
FORMS = ["host", "device"]
MANIFEST = Z.manifest()
NAMES = sorted(MANIFEST["fixtures"])


@pytest.fixture(scope="module")
def want():   # the plains, computed once, checked against the manifest and left alone
    plains = {**Z.plains(), "five_a": b"AAAAA"}
    for name, entry in MANIFEST["fixtures"].items():
        plain = plains[entry["plain"]]
        assert (len(plain), zlib.crc32(plain)) == (entry["length"], entry["crc32"]), "the plain of %s is not the one that was compressed" % name
    return {name: plains[entry["plain"]] for name, entry in MANIFEST["fixtures"].items()}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_one_frame_a_call(ctx, want, name, form):
    got, status, bad = Z.run(ctx, [Z.frame(name)], [len(want[name])], form)
    assert (status, bad) == ([0], 0) and got[0] == want[name]


@pytest.mark.parametrize("form", FORMS)
def test_all_frames_in_one_call(ctx, want, form):
    got, status, bad = Z.run(ctx, [Z.frame(k) for k in NAMES], [len(want[k]) for k in NAMES], form)
    assert bad == 0 and status == [0] * len(NAMES)
    assert [k for k, g in zip(NAMES, got) if g != want[k]] == []


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("patch", MANIFEST["patches"], ids=lambda p: p[3])
def test_malformed_frame_between_two_good_ones(ctx, want, patch, form):
    name, at, byte, cause = patch
    frame = bytearray(Z.frame(name))
    frame[at] = byte
    names = ["words_200_l1", name, "constant_5000_l1"]
    frames = [Z.frame(names[0]), bytes(frame), Z.frame(names[2])]
    got, status, bad = Z.run(ctx, frames, [len(want[k]) for k in names], form)
    assert status == [0, Z.CAUSES[cause], 0] and bad == 1 and got[1] == bytes(len(want[name]))
    assert got[0] == want[names[0]] and got[2] == want[names[2]]
    with pytest.raises(_capi.OxenError, match="block 1: " + cause):
        tabular.zstd_inflate(frames, sizes=[len(want[k]) for k in names], ctx=ctx)


@pytest.mark.parametrize("form", FORMS)
def test_more_frames_than_the_grid(ctx, want, form):
    """3 000 small frames over a grid capped at 512 waves: the frame loop's later rounds, a wave's tables and literal
    slot used again by frames of other forms."""
    cycle = ["words_200_l1", "rle_literals_no_sequence", "words_900_l3", "one_byte_l1", "skewed_low_l19", "constant_5000_l1", "words_900_window"]
    names = [cycle[k % len(cycle)] for k in range(3000)]
    got, status, bad = Z.run(ctx, [Z.frame(k) for k in names], [len(want[k]) for k in names], form)
    assert bad == 0 and not any(status) and got == [want[k] for k in names]


def test_list_form_and_a_frame_without_content_size(ctx, want):
    sized, bare = "words_900_checksum", "words_900_window"
    assert tabular.zstd_inflate([Z.frame(sized), Z.frame("empty_l1")], ctx=ctx) == [want[sized], b""]
    assert tabular.zstd_inflate([Z.frame(sized), Z.frame(bare)], sizes=[900, 900], ctx=ctx) == [want[sized], want[bare]]
    with pytest.raises(_capi.OxenError, match="block 1 carries no content size"):
        tabular.zstd_inflate([Z.frame(sized), Z.frame(bare)], ctx=ctx)
