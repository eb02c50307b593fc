"""The planted-boundary generator (tests/_cdc_plant.py) against the FastCDC oracle, on the CPU.

What tests/test_gpu_cdc_lattice.py feeds the device is only as good as this generator: here every
planted file's promise is checked against the C oracle length for length, every decoy is checked to be
what it claims, the two restatements of the oracle (the C one and chunks_py) meet on exactly the edges
random data misses, and the planner's coverage table is asserted so that a later edit cannot hollow
the device lattice out.
"""
import numpy as np
import pytest

import _cdc_plant as P
from oracle import fastcdc as F

CONFIG_IDS = [P.cfg_id(c) for c in P.CONFIGS]


def _lens(data, cfg, level=1):
    return F.chunks(data, *cfg, level)[:, 1].tolist()


def _assert_promise(pl, cfg, level=1):
    got = _lens(pl.data, cfg, level)
    if got != pl.lens:
        k = next((i for i, (g, w) in enumerate(zip(got, pl.lens)) if g != w), min(len(got), len(pl.lens)))
        pytest.fail(f"{P.cfg_id(cfg)} level {level}: chunk {k} ({pl.labels[k]!r}, start {pl.starts[k]}): "
                    f"promised {pl.lens[k]}, the oracle cuts {got[k] if k < len(got) else None}")
    assert sum(pl.lens) == len(pl.data)


def _assert_absent_justified(pl, cfg):
    """A planned length may be missing only where no trigger can exist: L = a0 + j, j <= 2 (the search over
    its j+1 hashed bytes is exhaustive), or a position cut_gear never tests (q >= eL)."""
    a0, eS, eL = P.geometry(cfg, cfg[2] + 1)
    for label, L, why in pl.absent:
        assert (a0 <= L <= a0 + 2 and why.startswith("no value")) or (eL <= L < cfg[2] and why.startswith("never")), \
            (P.cfg_id(cfg), label, L, why)


def test_roll_and_full_window_match_their_definitions(oracle_lib):
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 400, dtype=np.uint8)
    gear = F.gear_table()
    for a0 in (0, 7, 64):
        h, want = 0, []
        for b in data[a0:].tolist():
            h = ((h << 1) + gear[b]) & F.M64
            want.append(h)
        assert P.roll(data, a0).tolist() == want
    for p in (0, 5, 47, 48, 63, 64, 200, 399):
        w48 = 0
        for b in data[max(0, p - 47):p + 1].tolist():
            w48 = ((w48 << 1) + gear[b]) & F.M64
        got = int(P.full(data, p, p + 1)[0])
        assert got & ((1 << 48) - 1) == w48 & ((1 << 48) - 1)  # a 48-byte window decides every bit below 48
        assert got == int(P.full(data)[p])


@pytest.fixture(scope="module")
def lattices(oracle_lib):
    """Level 1, every config: what the device tests run over (built once)."""
    out = {}
    for cfg in P.CONFIGS:
        out[cfg] = {"length": P.length_lattice(cfg), "length-zero": P.length_lattice(cfg, filler="zero"),
                    "tail": P.tail_lattice(cfg), "position": P.position_lattice(cfg, P.min_section(cfg))}
        if P.min_section(cfg) < 65536:  # the lattice of the run at 64 KiB sections
            out[cfg]["position-64k"] = P.position_lattice(cfg, 65536)
    for cfg, path in P.DEFAULT_CASES:
        out[cfg][f"default-{path}"] = P.default_lattice(cfg, path)
    return out


def _position_keys():
    return [(cfg, "position") for cfg in P.CONFIGS] + [(cfg, "position-64k") for cfg in P.CONFIGS if P.min_section(cfg) < 65536]


@pytest.mark.parametrize("cfg", P.CONFIGS, ids=CONFIG_IDS)
def test_planted_lattices_keep_their_promise(lattices, cfg, capsys):
    absent = {}
    for name, lat in lattices[cfg].items():
        _assert_promise(lat.planted, cfg)
        _assert_absent_justified(lat.planted, cfg)
        absent[name] = [f"{label} (L={L}: {why})" for label, L, why in lat.planted.absent]
        assert len(lat.offs) == len(lat.lens) == len(lat.names)
        assert int((lat.offs + lat.lens).max()) <= len(lat.planted.data)
    with capsys.disabled():
        print(f"\n{P.cfg_id(cfg)}: absent lengths {absent}")
    # every j in 3..49 of the truncated-window class is there, plain and with decoys, for every filler
    a0 = P.geometry(cfg, cfg[2] + 1)[0]
    for name in ("length", "length-zero"):
        pl = lattices[cfg][name].planted
        for suffix in ("", " +decoys"):
            for j in range(3, 50):
                i = pl.labels.index(f"trunc j={j}{suffix}")
                assert pl.lens[i] == a0 + j, (name, j, suffix)
    # the filler modes plant the same lengths
    assert lattices[cfg]["length"].planted.lens == lattices[cfg]["length-zero"].planted.lens


@pytest.mark.parametrize("level", [0, 2, 3])
@pytest.mark.parametrize("cfg", P.CONFIGS, ids=CONFIG_IDS)
def test_planted_lengths_at_every_level(oracle_lib, cfg, level):
    lat = P.length_lattice(cfg, level=level)
    _assert_promise(lat.planted, cfg, level)
    _assert_absent_justified(lat.planted, cfg)
    a0 = P.geometry(cfg, cfg[2] + 1)[0]
    for j in range(3, 50):
        assert lat.planted.lens[lat.planted.labels.index(f"trunc j={j}")] == a0 + j


def test_zero_filler_leaves_no_candidates_but_the_planted(lattices):
    """F1 records a position when the bits both masks share are clear. The zero filler has such positions
    only where the planter wrote bytes: within 64 bytes after a re-drawn, trigger or decoy byte."""
    cfg = P.CONFIGS[0]
    pl = lattices[cfg]["length-zero"].planted
    ms, ml = F.masks(cfg[1])
    cand = (P.full(pl.data) & np.uint64(ms & ml)) == 0
    near = np.zeros(len(pl.data), dtype=bool)
    for p in np.flatnonzero(pl.data):
        near[p:p + 64] = True
    assert not (cand & ~near).any()
    rnd = lattices[cfg]["length"].planted
    assert ((P.full(rnd.data) & np.uint64(ms & ml)) == 0).sum() > 100  # the random filler: many false candidates


@pytest.mark.parametrize("cfg", P.CONFIGS, ids=CONFIG_IDS)
def test_decoys_are_what_they_claim(lattices, cfg):
    ms, ml = (np.uint64(m) for m in F.masks(cfg[1]))
    a0, eS, eL = P.geometry(cfg, cfg[2] + 1)
    kinds = set()
    for name in ("length", "length-zero", "position"):
        pl = lattices[cfg][name].planted
        cuts = set(np.cumsum(F.chunks(pl.data, *cfg)[:, 1]).tolist())
        for kind, pos, cs in pl.decoys:
            q = pos - cs
            mask = np.uint64(P.mask_at(cfg, 1, q))
            assert cs in cuts or cs == 0
            assert pos not in cuts, (name, kind, pos)  # the oracle does not cut there
            fw = P.full(pl.data, pos, pos + 1)[0]
            if kind == "a":
                tr = P.roll(pl.data[cs:pos + 1], a0)[-1]
                assert a0 + P.HASH_SPAN <= q < eS and tr & ml == 0 and tr & ms != 0 and fw & ml == 0
            elif kind == "b":
                assert 0 < q < a0 and fw & ms == 0
            else:
                tr = P.roll(pl.data[cs:pos + 1], a0)[-1]
                assert a0 <= q < a0 + P.HASH_SPAN and fw & mask == 0 and tr & mask != 0
            kinds.add(kind)
    want = {"b", "c"} | ({"a"} if a0 + P.HASH_SPAN + 17 < eS else set())
    assert kinds >= want, (kinds, want)
    # the plain truncated-window cuts are hidden from the full-window hash, the last position (j = 46,
    # where only bit 47 tells the two hashes apart) among them
    for name in ("length", "length-zero"):
        pl = lattices[cfg][name].planted
        js = set()
        for cut, cs in pl.hidden:
            mask = np.uint64(P.mask_at(cfg, 1, cut - cs))
            assert P.roll(pl.data[cs:cut + 1], a0)[-1] & mask == 0 and P.full(pl.data, cut, cut + 1)[0] & mask != 0
            js.add(cut - cs - a0)
        # (byte a0-1 enters position a0+j shifted by j+1: it can hide the cut where the mask has a bit there)
        can = {j for j in range(3, P.HASH_SPAN) if P.mask_at(cfg, 1, a0 + j) >> (j + 1)}
        assert js >= can, (name, sorted(can - js))
        assert P.HASH_SPAN - 1 in js or cfg[1] < 4096


@pytest.mark.parametrize("cfg", [P.CONFIGS[3], P.CONFIGS[4], P.CONFIGS[0]], ids=lambda c: P.cfg_id(c))
def test_two_restatements_agree_on_planted_edges(lattices, cfg):
    """chunks_py (per byte) and the C oracle (two bytes per step) on the planted files of the small configs
    and on the 8 KiB config's length lattice: the edges random data reaches with probability 2^-13."""
    names = ("length",) if cfg == P.CONFIGS[0] else ("length", "length-zero", "tail", "position")
    for name in names:
        lat = lattices[cfg][name]
        data = lat.planted.data.tobytes()
        assert [ln for _, ln in F.chunks_py(data, *cfg)] == lat.planted.lens, name
        if cfg != P.CONFIGS[0]:  # and item by item (the tails: rem <= min, center = rem, odd rem)
            for o, n in zip(lat.offs.tolist(), lat.lens.tolist()):
                item = data[o:o + n]
                assert [ln for _, ln in F.chunks_py(item, *cfg)] == _lens(np.frombuffer(item, np.uint8), cfg), (name, o, n)


def test_coverage_of_the_device_lattice(lattices, capsys):
    """The planner's coverage table: every class the device lattice names has planted cuts."""
    lines = []
    for cfg in P.CONFIGS:
        a0, eS, eL = P.geometry(cfg, cfg[2] + 1)
        L = lattices[cfg]
        cov = L["length"].coverage
        lines.append(f"{P.cfg_id(cfg):>18} length   " + "; ".join(f"{k}: {','.join(v)}" for k, v in cov.items()))
        # (min > avg puts `center` below a0: every tested position uses mask_l and there is no center class)
        classes = ("trunc", "center", "max", "mid") if cfg[1] + 2 >= a0 else ("trunc", "max", "mid")
        assert {c for c, _, _ in P.length_classes(cfg)} == set(classes)
        for cls in classes:
            assert {"plain", "decoys", "cut@first", "cut@last"} <= set(cov[cls]), (cfg, cls, cov[cls])
        events = set().union(*(set(cov[c]) for c in classes))
        assert {f"{x}@{e}" for x in ("a0", "a0+47", "center", "cut") for e in ("first", "last")} <= events, (cfg, events)
        assert [int(o) % 128 for o in L["length"].offs[1:]] == list(P.ITEM_PHASES)
        labels = set(L["length"].planted.labels)
        for _, label, Lc in P.length_classes(cfg):
            assert label in labels and label + " +decoys" in labels
        tc = L["tail"].coverage
        lines.append(f"{'':>18} tail     {tc}")
        for k in ("t<=min", "odd t, match at t-1", "even t, match at t-1", "t>max", "t==max"):
            assert tc[k] > 0, (cfg, k)
        assert tc["center=rem<avg"] > 0 or cfg[1] <= cfg[0] + 3, cfg
        ts = {int(n.split()[0][2:]) for n in L["tail"].names}
        missing = [t for t in P.tail_lengths(cfg) if t not in ts]
        assert not missing, (cfg, missing)
        for key in ("position", "position-64k"):
            if key not in L:
                assert P.min_section(cfg) >= 65536
                continue
            pc = L[key].coverage
            lines.append(f"{'':>18} {key} {pc}")
            assert pc["section"] == pc["unit"] == len(P.D_OFFSETS) and pc["group"] == 2
            if key == "position" and P.min_section(cfg) == cfg[2]:
                assert pc["run-last"] >= 8 and pc["run-first"] >= 8
            if a0 + P.HASH_SPAN + 33 < eS:
                assert pc["after-stored-candidate"] == 1
    for cfg, path in P.DEFAULT_CASES:
        dc = lattices[cfg][f"default-{path}"].coverage
        lines.append(f"{P.cfg_id(cfg):>18} default-{path} {dc}")
        # every offset where 8 MiB hold that many sections, and never fewer than the six window offsets
        fits = ((8 << 20) - (1 << 18)) // P.default_sections(cfg, path)
        assert dc["default-section"] >= min(len(P.D_OFFSETS), fits) and dc["default-section"] >= 6
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("cfg,key", _position_keys(), ids=lambda v: P.cfg_id(v) if isinstance(v, tuple) else v)
def test_position_lattice_puts_cuts_where_it_says(lattices, cfg, key):
    """Both position lattices -- the smallest sections and, built for it, 64 KiB sections (units of 1 KiB):
    every d of D_OFFSETS at a k*sec and at a k*unit of the section size the run uses."""
    sec = P.min_section(cfg) if key == "position" else 65536
    unit = sec // 64
    pl = lattices[cfg][key].planted
    ends = {lab: s + ln for s, ln, lab in zip(pl.starts, pl.lens, pl.labels)}
    seen = {"sec": set(), "unit": set()}
    for lab, e in ends.items():
        w = lab.split()
        if w[0] in ("sec", "unit"):
            k, d = int(w[1][2:]), int(w[2][2:])
            assert e == k * (sec if w[0] == "sec" else unit) + d, lab
            seen[w[0]].add(d)
        elif w[0] == "group":
            assert e % 16 == int(w[2][3:]), lab
    assert seen["sec"] == seen["unit"] == set(P.D_OFFSETS)
    # the unit anchors are no section anchors in disguise
    assert all(int(lab.split()[1][2:]) % 64 for lab in ends if lab.startswith("unit "))
    # the cut after a stored candidate: the decoy is an F1 candidate (the bits both masks share are clear in
    # its full-window hash) in the first 16-byte group of its unit, so no group of that unit is stored
    # before it; the cut lies in the unit's second group
    lab = "cut in the group after a stored candidate"
    a0, eS, _ = P.geometry(cfg, cfg[2] + 1)
    assert (lab in ends) == (a0 + P.HASH_SPAN + 33 < eS)
    if lab in ends:
        cs = pl.starts[pl.labels.index(lab)]
        (kind, pos, dcs), = [d for d in pl.decoys if d[2] == cs]
        ms, ml = F.masks(cfg[1])
        assert kind == "a" and pos % unit == P.AFTER_STORED[0] < 16 and P.full(pl.data, pos, pos + 1)[0] & np.uint64(ms & ml) == 0
        assert ends[lab] % unit == P.AFTER_STORED[1] and 16 <= P.AFTER_STORED[1] < 32 and ends[lab] // unit == pos // unit
    if key == "position" and sec == cfg[2]:
        for name, ph in (("last", sec - 1), ("first", 0)):
            starts = [s for s, lab in zip(pl.starts, pl.labels) if lab.startswith(f"run-{name} ") and "lead" not in lab]
            assert len(starts) == 9 and all(s % sec == ph for s in starts)
            assert np.diff(starts).tolist() == [sec] * 8  # one start in each of nine consecutive sections


@pytest.mark.parametrize("cfg,path", P.DEFAULT_CASES, ids=lambda v: P.cfg_id(v) if isinstance(v, tuple) else v)
def test_default_lattice_puts_cuts_at_the_derived_sections(lattices, cfg, path):
    """The files of the runs without a section override: promise kept (test_planted_lattices_keep_their_promise
    covers them), one cut at k*sec + d for consecutive k from 1, sec the size the device entry derives, the
    offsets the first of D_BY_WEIGHT, the file under 8 MiB."""
    sec = P.default_sections(cfg, path)
    assert sec == {"scan": max(512 << 10, 8 * cfg[2]), "walk": max(64 << 10, 4 * cfg[2])}[path]
    pl = lattices[cfg][f"default-{path}"].planted
    _assert_promise(pl, cfg)
    assert len(pl.data) < 8 << 20
    got = [(int(lab.split()[1][2:]), int(lab.split()[2][2:]), s + ln)
           for s, ln, lab in zip(pl.starts, pl.lens, pl.labels) if lab.startswith("default-sec")]
    assert [k for k, _, _ in got] == list(range(1, len(got) + 1))
    assert [d for _, d, _ in got] == list(P.D_BY_WEIGHT[:len(got)]) and sorted(P.D_BY_WEIGHT) == sorted(P.D_OFFSETS)
    assert all(e == k * sec + d for k, d, e in got)
    assert len(got) == len(P.D_OFFSETS) or (len(got) + 1) * sec + cfg[2] + cfg[0] + 49 >= 8 << 20  # as many as fit


def test_prefix_and_anchors(oracle_lib):
    cfg = P.CONFIGS[0]
    plan = [P.Cut(at=400_000, label="x"), 5000, P.Random(until=600_000), P.Cut(at=700_001, label="y", decoys="abc")]
    pl = P.plant(cfg, 1, plan, seed=9, prefix=300_000)
    _assert_promise(pl, cfg)
    ends = {lab: s + ln for s, ln, lab in zip(pl.starts, pl.lens, pl.labels)}
    assert ends["x"] == 400_000 and ends["y"] == 700_001
    assert pl.labels.count("random") > 20 and pl.starts[pl.labels.index("fill")] >= 300_000


@pytest.mark.parametrize("cfg", [P.CONFIGS[0], P.CONFIGS[1]], ids=lambda c: P.cfg_id(c))
def test_segment_edge_files_scaled_down(oracle_lib, cfg):
    """The files of the host-pipeline test with the segment ends pulled in to 1 MiB and 2 MiB - max: every
    case at both ends keeps its promise and puts its chunk starts where its name says."""
    mx = cfg[2]
    ends = [1 << 20, (2 << 20) - mx]
    for c in range(len(P.EDGE_CASES)):
        pl = P.edge_file(cfg, ends, [c, (c + 3) % len(P.EDGE_CASES)], (2 << 20) + 300_001, seed=c)
        _assert_promise(pl, cfg)
        E = ends[0]
        starts = set(pl.starts)
        want = {0: [E - mx, E], 1: [E - mx, E], 2: [E - mx + 1, E - 1], 3: [E - mx - 1, E + 1],
                4: [E - cfg[0] - 23, E - 13], 5: [E - cfg[0] - 23, E + 17], 6: [E - mx + 1, E], 7: [E - mx - 1, E - 1]}[c]
        assert all(s in starts for s in want), (c, want)
