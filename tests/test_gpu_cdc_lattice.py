"""The FastCDC kernels (F1 scan, F2 walk, F3 stitch, W, X) and the host pipeline's stitcher on planted
chunk boundaries (tests/_cdc_plant.py, which says which code path each class of case is for and is
pinned on the oracle by tests/test_cdc_plant.py).

tests/test_fastcdc.py feeds the chunker random, text-like and constant bytes: a statistical net. Here
the cuts are put where the kernels branch -- every position of the truncated window, center-2 ..
center+2, max-2 .. max, the parity rule, section / unit / group / 128-byte line boundaries at offsets
-49 .. +49, false candidates of three kinds, tails of every length class, and the host pipeline's
segment ends -- on both chunking paths: "scan" (OXH_CDC_WALK=0: F1 + F2 + F3) for every config and
"walk" (OXH_CDC_WALK=1: W + X, which fails loudly where it cannot be taken) for the configs whose masks
sit at bit 16 or above. Every item's chunk table must equal F.chunks of its bytes and every digest the
oracle's; a mismatch names the config, the path, the planner's class of the first wrong chunk, its
start and the two lengths.
"""
import os
import time

import numpy as np
import pytest

import _cdc_plant as P
from oracle import fastcdc as F
from test_fastcdc import _check_items, _check_table

CASES = [(cfg, "scan") for cfg in P.CONFIGS] + [(cfg, "walk") for cfg in P.WALK_CONFIGS]
CASE_IDS = [f"{P.cfg_id(c)}-{p}" for c, p in CASES]
KNOBS = ("OXH_CDC_WALK", "OXH_CDC_SECTION_BYTES", "OXH_CDC_WARMUP_BYTES", "OXH_CDC_UNIT_CAP")


@pytest.fixture(scope="module")
def planted():
    """The lattices, built once per module on first use: get(kind, cfg, *args)."""
    cache = {}
    build = {"length": P.length_lattice, "tail": P.tail_lattice, "position": P.position_lattice,
             "default": P.default_lattice}

    def get(kind, cfg, *args, **kw):
        key = (kind, cfg, args, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = build[kind](cfg, *args, **kw)
        return cache[key]

    return get


def _path(monkeypatch, path, **knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("OXH_CDC_WALK", "1" if path == "walk" else "0")
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))


def _run(cuda, oracle_lib, lat, cfg, path, what):
    pl = lat.planted

    def explain(i, want, got_off, got_len):
        return (f"{P.cfg_id(cfg)} {path} {what}, item {lat.names[i]!r} at arena offset {int(lat.offs[i])}: "
                + P.explain(pl, int(lat.offs[i]), want, got_off, got_len))

    # the planter's promise (pinned on the CPU by test_cdc_plant.py; cheap enough to hold here too)
    assert F.chunks(pl.data, *cfg)[:, 1].tolist() == pl.lens, f"{what}: the planted file does not keep its promise"
    t0 = time.perf_counter()
    n = _check_items(cuda, oracle_lib, pl.data, lat.offs, lat.lens, *cfg, explain=explain)
    print(f"{P.cfg_id(cfg)} {path} {what}: {len(lat.offs)} items, {int(lat.lens.sum())} B, {n} chunks, "
          f"{time.perf_counter() - t0:.2f} s")
    assert n >= len(lat.offs)


@pytest.mark.gpu
@pytest.mark.parametrize("filler", ["random", "zero"])
@pytest.mark.parametrize("cfg,path", CASES, ids=CASE_IDS)
def test_cdc_length_lattice(cuda, oracle_lib, monkeypatch, planted, cfg, path, filler):
    """Every length class (a0 + 0..49, center-2 .. center+2, max-2 .. max, two mid-range lengths), each once
    plain and once with decoys (a), (b), (c) attached, at chunk-start phases that put cs+a0, cs+a0+47,
    cs+center and the cut on the first and the last byte of a 128-byte line; the chain as one item and as
    six items that start 0, 1, 15, 16, 64 and 127 bytes past a 128-byte boundary of the arena. The random
    filler leaves many false F1 candidates, the zero filler none but the planted ones."""
    _path(monkeypatch, path)
    _run(cuda, oracle_lib, planted("length", cfg, filler=filler), cfg, path, f"length lattice ({filler} filler)")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,path", CASES, ids=CASE_IDS)
def test_cdc_tail_lattice(cuda, oracle_lib, monkeypatch, planted, cfg, path):
    """Items that end t bytes after a chunk start, for every t in min-1 .. min+50, avg-2 .. avg+2 and
    max-2 .. max+2, with a match planted at t-1, t-2 or t-3: `rem <= min`, the last tested position, the
    first untested one (odd rem), center = rem < avg, rem around max."""
    _path(monkeypatch, path)
    _run(cuda, oracle_lib, planted("tail", cfg), cfg, path, "tail lattice")


def _position_variants():
    out = []
    for cfg, path in CASES:
        sec = P.min_section(cfg)
        v = [("min-sections", sec, {}), ("min-sections-nowarmup", sec, {"OXH_CDC_WARMUP_BYTES": 0})]
        if sec < 65536:  # (above that the override is raised to `max`: the run above once more)
            v.append(("64KiB-sections", 65536, {}))
        if path == "scan":
            v.append(("min-sections-cap1", sec, {"OXH_CDC_UNIT_CAP": 1}))
        out += [pytest.param(cfg, path, name, s, knobs, id=f"{P.cfg_id(cfg)}-{path}-{name}") for name, s, knobs in v]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,path,name,sec,knobs", _position_variants())
def test_cdc_position_lattice(cuda, oracle_lib, monkeypatch, planted, cfg, path, name, sec, knobs):
    """Cuts anchored at k*sec + d and k*unit + d, d in -49 .. +49, at 16*g + 0 and + 15, in the group after
    a unit's stored candidate, and (sec == max) runs of max-sized chunks that start on the last, then on
    the first byte of nine consecutive sections -- with the smallest sections the config allows (the
    override 8192 is raised to `max` rounded up to 8 KiB: units of 128 or 256 bytes at the small configs),
    the same without warm-up (most sections fail convergence: F3b, X's retry and fix passes re-walk them),
    with one stored candidate per unit (the walk scans the bytes after it), and a lattice of its own, built
    for that section size, at 64 KiB sections (units of 1 KiB). OXH_CDC_SECTION_BYTES is the section the
    lattice was built for (min_section rounds as the device entry does, so the value holds as given)."""
    assert sec % 8192 == 0 and sec >= cfg[2]
    _path(monkeypatch, path, OXH_CDC_SECTION_BYTES=sec, **knobs)
    _run(cuda, oracle_lib, planted("position", cfg, sec), cfg, path, f"position lattice ({name})")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,path", P.DEFAULT_CASES, ids=lambda v: P.cfg_id(v) if isinstance(v, tuple) else v)
def test_cdc_default_section_plans(cuda, oracle_lib, monkeypatch, planted, cfg, path):
    """No section override: cuts anchored around the boundaries of the sections oxh_fastcdc_device derives
    for a small input (P.default_sections restates its sizing: 512 KiB or 8 max for the scan, 64 KiB or
    4 max for the walk); the file stays under 8 MiB so that the walk's byte-count term stays below that."""
    _path(monkeypatch, path)
    _run(cuda, oracle_lib, planted("default", cfg, path), cfg, path, "default sections")


# ------------------------------------------------------------------------------ host pipeline
PIECE = 64 << 20


def _segment_ends(size: int, mx: int, piece: int = PIECE) -> list:
    """Where a single file's segments end, as the plan loop of the host entries cuts them (fastcdc_host.cpp,
    "plan: files in order into this piece"): a file that does not fit what is left of a piece takes all of
    it (here the whole piece, which is at least the 16 MiB a segment needs) and goes on `max` bytes
    before that end, so that the carried chunk start lies in the next segment."""
    ends, lo = [], 0
    while size - lo > piece:
        ends.append(lo + piece)
        lo += piece - mx
    return ends


EDGE_FILES = [(0, 1), (3, 2), (4, 5), (7, 6)]  # the EDGE_CASES planted at (E1, E2) of each file


@pytest.mark.gpu
@pytest.mark.parametrize("pair", EDGE_FILES, ids=lambda p: f"cases{p[0]}{p[1]}")
@pytest.mark.parametrize("cfg", [P.CONFIGS[0], P.CONFIGS[1]], ids=lambda c: P.cfg_id(c))
def test_cdc_host_segment_edges(cuda, oracle_lib, monkeypatch, tmp_path, cfg, pair):
    """stitch() carries a chunk when pos + max > E, keeps it when pos + max == E, and sets carry = E when
    every chunk of the segment is final. With OXH_CDC_PIECE_MIB=64 a 130 MiB file's segments end at
    E1 = 64 MiB and E2 = 128 MiB - max (nothing smaller is reachable: the piece is at least 2 x 16 MiB
    rounded up to whole 64 MiB bounce windows). The file is random except near E1 and E2, where one of
    P.EDGE_CASES each is planted; the whole file's boundaries and digests equal the oracle's, through
    fastcdc_host on both paths and (one file) through fastcdc_files."""
    from oxen_amd import dedup

    assert int(os.environ.get("OXH_CDC_BOUNCE_MIB") or 64) <= 64, "the 64 MiB piece needs bounce windows of at most 64 MiB"
    mx = cfg[2]
    size = (130 << 20) + 12_345 + 1_001 * pair[0]
    ends = _segment_ends(size, mx)
    assert ends == [64 << 20, (128 << 20) - mx]
    pl = P.edge_file(cfg, ends, pair, size, seed=100 + pair[0])
    assert _segment_ends(len(pl.data), mx) == ends
    want = F.chunks(pl.data, *cfg)
    assert want[:, 1].tolist() == pl.lens  # the planted promise, at full size
    starts = set(pl.starts)
    for E, c in zip(ends, pair):  # the chunk starts the cases are named after
        near = {0: [E - mx, E], 1: [E - mx, E], 2: [E - mx + 1, E - 1], 3: [E - mx - 1, E + 1],
                4: [E - 13], 5: [E + 17], 6: [E - mx + 1, E], 7: [E - mx - 1, E - 1]}[c]
        assert all(s in starts for s in near), (E, c, P.EDGE_CASES[c])
    monkeypatch.setenv("OXH_CDC_PIECE_MIB", "64")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def check(tab, how):
        off, ln, _ = tab.file(0)
        if not (len(off) == len(want) and np.array_equal(off, want[:, 0]) and np.array_equal(ln, want[:, 1])):
            pytest.fail(f"{P.cfg_id(cfg)} {how}, segment ends {ends}, cases {[P.EDGE_CASES[c] for c in pair]}: "
                        + P.explain(pl, 0, want, off, ln))
        _check_table(oracle_lib, tab, [pl.data], *cfg)

    for path in (("walk", "scan") if cfg == P.CONFIGS[0] else ("scan",)):
        monkeypatch.setenv("OXH_CDC_WALK", "1" if path == "walk" else "0")
        t0 = time.perf_counter()
        tab = dedup.fastcdc_host([pl.data], *cfg)
        print(f"{P.cfg_id(cfg)} {path} fastcdc_host {len(pl.data)} B: {time.perf_counter() - t0:.2f} s")
        check(tab, f"fastcdc_host {path}")
    if pair == EDGE_FILES[0] and cfg == P.CONFIGS[0]:
        monkeypatch.delenv("OXH_CDC_WALK")
        p = tmp_path / "edges"
        pl.data.tofile(str(p))
        tab = dedup.fastcdc_files([str(p)], *cfg)
        assert list(tab.status) == [0] and list(tab.sizes) == [len(pl.data)]
        check(tab, "fastcdc_files")
