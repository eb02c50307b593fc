"""The length-by-alignment lattice the wave kernels are checked on (tests/test_gpu_lattice.py), and the
oracle is pinned on (tests/test_oracle.py, tests/golden/lattice.json).

K1's path (xxh3_kernels.hip wave_long, rows_item) depends on bs = start & 3, on nb & 3 (which blocks of
the final round are full), on ns (0..15), on len - E (1..64, with the switch bs && len - E >= 4), and on
nr against the ring depth D (2 for variants 8/72/104, 4 for variant 0):

  LENS    every L in 0..8192 (nr 0 and 1, every nb & 3, ns and len - E at both), and
          L = (4*nr + m)*1024 + r for nr in NR (D-1, D, D+1, 2D, 2D+1 for both depths), m in 0..3, r in R
  SHIFTS  every bs, and two starts off 16-byte alignment

Items overlap in one arena of SPAN = max(LENS) + 16 bytes: item (s, L) is arena[s : s + L], shift-major
(all lengths at shift SHIFTS[0], then SHIFTS[1], ...). 53 046 items hash ~0.3 GB out of ~40 KiB.
"""
import hashlib

import numpy as np

SEED = 0x1A771CE
NR = (2, 3, 4, 5, 8, 9)
R = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 66, 67, 68, 127, 128, 129, 512, 513, 960, 961, 963, 964, 1021, 1022,
     1023, 1024]
DENSE_TO = 8192
SHIFTS = [0, 1, 2, 3, 8, 13]
LENS = np.array(list(range(DENSE_TO + 1)) + [(4 * nr + m) * 1024 + r for nr in NR for m in range(4) for r in R],
                dtype=np.uint64)
SPAN = int(LENS.max()) + 16
N = len(LENS) * len(SHIFTS)


def definition() -> dict:
    """What lattice.json records beside the digests: a change here without regenerating it fails the pin."""
    return {"seed": SEED, "dense_to": DENSE_TO, "nr": list(NR), "m": [0, 1, 2, 3], "r": list(R), "shifts": list(SHIFTS),
            "span": SPAN, "items_per_shift": len(LENS), "order": "shift-major; item (s, L) = arena[s : s + L]",
            "arena": "splitmix_bytes(seed, 0, span)"}


def items():
    """(offsets, lens) of every item, uint64, shift-major."""
    offs = np.repeat(np.array(SHIFTS, dtype=np.uint64), len(LENS))
    return offs, np.tile(LENS, len(SHIFTS))


def shift_slice(k: int) -> slice:
    return slice(k * len(LENS), (k + 1) * len(LENS))


def host_arena(kind: str = "splitmix") -> np.ndarray:
    """The arena's bytes on the host: 'splitmix' (all 256 values), 'nl' (every byte 0x0A), 'cont' (0x80)."""
    if kind == "splitmix":
        from oxen_amd.workloads import splitmix_bytes

        return splitmix_bytes(SEED, 0, SPAN)
    return np.full(SPAN, {"nl": 0x0A, "cont": 0x80}[kind], dtype=np.uint8)


def device_arena(kind: str, device):
    """The same bytes in device memory; the random ones generated there (fill_splitmix, which
    test_fill_splitmix_matches_host ties to splitmix_bytes)."""
    import torch

    if kind == "splitmix":
        from oxen_amd.device import fill_splitmix

        assert SPAN % 8 == 0
        t = torch.empty(SPAN, dtype=torch.uint8, device=device)
        fill_splitmix(t, SEED)
        return t
    return torch.from_numpy(host_arena(kind)).to(device)


def text_counts(arena: np.ndarray, offs: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """(num_lines, num_chars) of every item from prefix sums over the host arena:
    lines = 1 + newlines, chars = bytes that are not UTF-8 continuation bytes (10xxxxxx)."""
    nl = np.concatenate([[0], np.cumsum(arena == 0x0A)]).astype(np.int64)
    cont = np.concatenate([[0], np.cumsum((arena & 0xC0) == 0x80)]).astype(np.int64)
    o, e = offs.astype(np.int64), (offs + lens).astype(np.int64)
    return np.stack([1 + nl[e] - nl[o], lens.astype(np.int64) - (cont[e] - cont[o])], axis=1)


def table_sha256(table: np.ndarray) -> list:
    """SHA-256 of the packed little-endian (lo, hi) digests of each shift's items."""
    t = np.ascontiguousarray(table, dtype="<u8")
    return [hashlib.sha256(t[shift_slice(k)].tobytes()).hexdigest() for k in range(len(SHIFTS))]


def mismatches(got: np.ndarray, want: np.ndarray, offs: np.ndarray, lens: np.ndarray, limit: int = 20,
               with_rows: bool = False):
    """(total, the first `limit` (shift, len) pairs) of the rows where got != want; with_rows: and
    those rows' indices."""
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(lens), -1).any(axis=1))[0]
    pairs = [(int(offs[i]), int(lens[i])) for i in bad[:limit]]
    return (len(bad), pairs, bad[:limit].tolist()) if with_rows else (len(bad), pairs)
