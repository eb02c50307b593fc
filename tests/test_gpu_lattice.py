"""K1, K1T, K1L and the fixed-chunk path on a full length-by-alignment lattice (tests/_lattice.py).

The wave kernels' risk is their edge arithmetic: partial rounds, partial blocks, the last stripe,
byte-shifted starts. The golden lengths give every length one start, so three quarters of the
(len mod 1024, start & 3) pairs never ran; here every length 0..8192 and the residues around every
ring-depth boundary run at every byte shift, in one batch per kernel shape. Everything is bit-exact
against the CPU oracle (pinned to libxxhash on the same lattice by test_oracle.py::test_lattice_golden)
or, for the text counts, against prefix sums over the host arena. No tolerances.
"""
import numpy as np
import pytest

import _lattice
from oxen_amd import _capi

pytestmark = pytest.mark.gpu

# The K1 shapes the shipped library instantiates, as in test_gpu_parity.py. 0 means "no forced variant": the
# dispatch then picks 8 for a WAVE batch, so the 4-round ring (Cfg<0>, the fallback of any forced variant
# that has no kernel) runs only under such a number; 392 is the one test_chunk_digests uses. 776 and 1032
# have the K1R bit and the bits of two experiments that are gone (git history has them): they too must run
# the 4-round ring at one item per wave, not K1R's launch geometry.
VARIANTS = [0, 8, 72, 104, 264]
RING4 = 392
RING4_FORMER = [776, 1032]
MODE_WAVE, MODE_LANE, MODE_SHORT, MODE_PACKED = (_capi.OXH_MODE_WAVE, _capi.OXH_MODE_LANE, _capi.OXH_MODE_WAVE_SHORT,
                                                  _capi.OXH_MODE_WAVE_PACKED)


def _u64(t):
    from oxen_amd.device import to_numpy_u64

    return to_numpy_u64(t).reshape(-1, 2)


def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to(cuda)


@pytest.fixture(scope="module")
def lattice(oracle_lib):
    """Items and their expected digests / text counts per arena kind, computed once on the host."""
    offs, lens = _lattice.items()
    offs.setflags(write=False)
    lens.setflags(write=False)
    want, counts = {}, {}
    for kind in ("splitmix", "nl", "cont"):
        host = _lattice.host_arena(kind)
        want[kind] = oracle_lib.batch(host, offs, lens, threads=16)
        counts[kind] = _lattice.text_counts(host, offs, lens)
        want[kind].setflags(write=False)
        counts[kind].setflags(write=False)
    # the constant arenas' counts in closed form: a byte read past either end, skipped or counted twice shows
    L = lens.astype(np.int64)
    assert np.array_equal(counts["nl"], np.stack([1 + L, L], axis=1))
    assert np.array_equal(counts["cont"], np.stack([np.ones_like(L), np.zeros_like(L)], axis=1))
    return {"offs": offs, "lens": lens, "want": want, "counts": counts}


@pytest.fixture(scope="module")
def arenas(cuda):
    return {kind: _lattice.device_arena(kind, cuda) for kind in ("splitmix", "nl", "cont")}


def _run_k1(cuda, arena, offs, lens, variant, mode):
    from oxen_amd.device import xxh3_128_batch_device

    prev = _capi.lib().oxh_set_kernel_variant(variant)
    try:
        return _u64(xxh3_128_batch_device(arena, _dev(offs, cuda), _dev(lens, cuda), mode=mode))
    finally:
        _capi.lib().oxh_set_kernel_variant(prev)


def _assert_digests(got, want, offs, lens, what):
    total, first = _lattice.mismatches(got, want, offs, lens)
    assert total == 0, f"{what}: {total} of {len(lens)} digests differ, first (shift, len): {first}"


@pytest.mark.parametrize("variant,order", [(v, o) for o in ("lattice", "permuted") for v in VARIANTS + [RING4]] +
                         [(v, "lattice") for v in RING4_FORMER])
def test_k1_wave_lattice(cuda, lattice, arenas, variant, order):
    """K1 (one wave per item; 264: K1R, a 16-lane row per item; 392, 776, 1032: the 4-round ring) over the
    whole lattice. In lattice order a K1R wave's four rows hold neighbouring lengths; permuted they hold very
    different ones, short (<= 240) items among long ones, in lockstep to the longest."""
    offs, lens, want = lattice["offs"], lattice["lens"], lattice["want"]["splitmix"]
    if order == "permuted":
        perm = np.random.default_rng(_lattice.SEED).permutation(len(lens))
        offs, lens, want = offs[perm], lens[perm], want[perm]
    got = _run_k1(cuda, arenas["splitmix"], offs, lens, variant, MODE_WAVE)
    _assert_digests(got, want, offs, lens, f"K1 variant {variant}, {order} order")


@pytest.mark.parametrize("mode", [MODE_LANE, MODE_SHORT, MODE_PACKED], ids=["lane", "short", "packed"])
def test_k1_modes_lattice(cuda, lattice, arenas, mode):
    """The lane kernel (K1s) and the SHORT / PACKED shapes the dispatch picks by itself (variant 0: no
    forced variant, so 72 and 104 run as the dispatch launches them)."""
    got = _run_k1(cuda, arenas["splitmix"], lattice["offs"], lattice["lens"], 0, mode)
    _assert_digests(got, lattice["want"]["splitmix"], lattice["offs"], lattice["lens"], f"mode {mode}")


@pytest.mark.parametrize("kind", ["splitmix", "nl", "cont"])
@pytest.mark.parametrize("variant", [0, 8])
def test_k1t_lattice(cuda, lattice, arenas, variant, kind):
    """K1T (text counts fused into K1) over the whole lattice: digests against the oracle, counts against
    prefix sums over the host arena. Random bytes (all 256 values); every byte 0x0A, where every item
    must report (1 + L, L); every byte 0x80, where every item must report (1, 0) -- so any byte the
    kernel misses, reads past either end of the item, or counts twice changes a count. A forced K1
    variant (8) must not change which K1T runs."""
    from oxen_amd.device import xxh3_128_text_batch_device

    offs, lens = lattice["offs"], lattice["lens"]
    prev = _capi.lib().oxh_set_kernel_variant(variant)
    try:
        out, counts = xxh3_128_text_batch_device(arenas[kind], _dev(offs, cuda), _dev(lens, cuda))
        got, cnt = _u64(out), counts.cpu().numpy()
    finally:
        _capi.lib().oxh_set_kernel_variant(prev)
    want_cnt = lattice["counts"][kind]
    total, first, rows = _lattice.mismatches(cnt, want_cnt, offs, lens, with_rows=True)
    detail = [(s, L, cnt[i].tolist(), want_cnt[i].tolist()) for (s, L), i in zip(first[:5], rows)]
    assert total == 0, (f"K1T on the {kind} arena: {total} of {len(lens)} (lines, chars) differ, first (shift, len): "
                        f"{first}; (shift, len, got, want): {detail}")
    _assert_digests(got, lattice["want"][kind], offs, lens, f"K1T on the {kind} arena")


CHUNKS = [241, 1021, 1027, 4099, 8197, 16387, 65537]


@pytest.fixture(scope="module")
def chunk_buffer(cuda, oracle_lib):
    """(1 << 20) + 123 random bytes on the device and on the host, and the oracle's chunk digests of the
    whole buffer and of the buffer from byte 1, per chunk size."""
    import torch

    from oxen_amd.device import fill_splitmix

    n = (1 << 20) + 123
    buf = torch.empty((n + 7) // 8 * 8, dtype=torch.uint8, device=cuda)
    fill_splitmix(buf, 78)
    host = buf[:n].cpu().numpy()
    want = {(start, c): oracle_lib.chunk_digests(host[start:], c, threads=16) for start in (0, 1) for c in CHUNKS}
    return buf, n, want


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("variant", [0, 264])
def test_chunk_digests_odd_sizes(cuda, chunk_buffer, variant, start):
    """Fixed-size chunks whose size is not a multiple of 4, so start & 3 cycles through every value from
    chunk to chunk (every size in test_chunk_digests keeps it 0); the buffer whole and viewed from byte 1;
    the default K1 shapes and K1R forced."""
    from oxen_amd.device import chunk_digests_device

    buf, n, want = chunk_buffer
    prev = _capi.lib().oxh_set_kernel_variant(variant)
    try:
        for chunk in CHUNKS:
            got = _u64(chunk_digests_device(buf[start:], chunk, nbytes=n - start))
            bad = np.nonzero((got != want[(start, chunk)]).any(axis=1))[0]
            assert len(bad) == 0, (f"chunk size {chunk} from byte {start}: {len(bad)} of {len(got)} chunks differ, "
                                   f"first chunk indices {bad[:20].tolist()}")
    finally:
        _capi.lib().oxh_set_kernel_variant(prev)


# K1L: block sums chip-wide (xxh3_blocksum_kernel), then the serial chain (xxh3_chain_kernel), which takes
# the block sums in groups of 256 steps and the remainder one by one, then the partial block's stripes and
# the last stripe in scalar code.
K1L_NB = [1024, 1025, 1279, 1280, 1281, 1282, 1537]  # the threshold (nb >= 1024); 1 + 256k steps -1, 0, +1, +2
K1L_R = [1, 2, 3, 4, 63, 64, 65, 1023, 1024] + [64 * s + 1 for s in range(2, 16)]  # every ns
K1L_SHIFTS = [0, 5, 16]
K1L_SPAN = 1538 * 1024 + 64  # arena bytes (~1.6 MiB): every item ends below (1537 + 1) KiB + 16


@pytest.fixture(scope="module")
def k1l_arena(cuda):
    import torch

    from oxen_amd.device import fill_splitmix

    arena = torch.empty(K1L_SPAN, dtype=torch.uint8, device=cuda)
    fill_splitmix(arena, 79)
    return arena, arena.cpu().numpy()


def _check_k1l(oracle_lib, arena, host, items, what):
    """items: (shift, len) views of the arena, one large_digests_device call, against oracle.batch."""
    import torch

    from oxen_amd.device import large_digests_device

    offs = np.array([s for s, _ in items], dtype=np.uint64)
    lens = np.array([n for _, n in items], dtype=np.uint64)
    assert int((offs + lens).max()) <= arena.numel()
    got = _u64(large_digests_device([arena[s:s + n] for s, n in items], [n for _, n in items]))
    torch.cuda.synchronize()
    want = oracle_lib.batch(host, offs, lens, threads=16)
    _assert_digests(got, want, offs, lens, what)


@pytest.mark.parametrize("nb", K1L_NB)
def test_k1l_lattice(cuda, oracle_lib, k1l_arena, nb):
    """K1L over overlapping views of one arena: L = nb * 1024 + r at every ns and tail residue, at three
    shifts -- 69 chained buffers per call, so the chain launches flush mid-round (kChainJobs = 32) --
    with buffers just below the threshold (nb = 1023: one K1 wave each) and an empty one among them."""
    arena, host = k1l_arena
    items = [(s, nb * 1024 + r) for s in K1L_SHIFTS for r in K1L_R]
    below = [(s, 1023 * 1024 + r) for s in K1L_SHIFTS for r in (1, 64, 1023, 1024)]
    items = items[:40] + below[:6] + [(0, 0)] + items[40:] + below[6:]
    assert sum(1 for _, n in items if (n - 1) >> 10 >= 1024) > 32
    _check_k1l(oracle_lib, arena, host, items, f"K1L nb {nb}")


@pytest.mark.parametrize("shift", [0, 5])
def test_k1l_piece_edges(cuda, oracle_lib, shift, monkeypatch):
    """K1L in 1 MiB pieces (OXH_BIG_PIECE_MIB=1): lengths around pieces_of()'s steps -- a last piece of
    1 025 B is the smallest with a scrambled block, so P + 1024 is one piece and P + 1025 two."""
    import torch

    from oxen_amd.device import fill_splitmix

    monkeypatch.setenv("OXH_BIG_PIECE_MIB", "1")
    P = 1 << 20
    sizes = [P + d for d in (1, 1023, 1024, 1025, 1026)] + [2 * P + 1024, 2 * P + 1025, 3 * P + 7]
    arena = torch.empty(3 * P + 64, dtype=torch.uint8, device=cuda)
    fill_splitmix(arena, 80)
    _check_k1l(oracle_lib, arena, arena.cpu().numpy(), [(shift, n) for n in sizes], f"K1L 1 MiB pieces, shift {shift}")
