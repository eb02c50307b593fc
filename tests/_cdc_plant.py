"""Planted FastCDC inputs: byte strings whose chunk boundaries fall where the planner wants them
(tests/test_cdc_plant.py pins this generator on the oracle; tests/test_gpu_cdc_lattice.py runs the
device chunker and the host pipeline over what it makes).

cut_gear (oracle/fastcdc_oracle.c) looks at a chunk that starts at `cs` like this: the hash starts
from 0 at a0 = 2*(min/2); position q in [a0, eL) is tested after byte cs+q went into the hash, against
mask_s while q < eS = 2*(center/2) and mask_l after it, eL = 2*(min(rem, max)/2); a match at q makes
the chunk q bytes long (byte q is the next chunk's first byte). The cut depends only on the bytes, so:

  clean     re-draw the byte at every tested position before L whose hash matches, until none does
  trigger   search the last 1-3 hashed bytes (L-2 .. L) for values that make position L match the
            mask that applies there, with L-2 and L-1 still not matching
  forced    L == max, or a length cut_gear never tests (q >= eL: max-1 when max is odd): clean up to
            eL and plant no trigger; the chunk is `max` long. An untestable length is reported in
            `absent`, and so is L = a0 + j, j <= 2, when no value of its j+1 hashed bytes matches.

What each class of planted case is for in oxen_amd/csrc/fastcdc_scan.hip and fastcdc_walk.hip:

  trunc     L = a0 + j, j = 0..49: cdc_cut's and X's truncated window (the 47 positions from a0 whose
            hash has not seen 48 bytes: the walks recompute them from the bytes), its last position
            (j = 46), the first positions that come from F1's candidates (j = 47, 48, 49), and with
            eS inside the window (avg = 4120) the mask switch in the exact loop. The plain ones are
            "hidden": byte a0-1 is chosen so that the full-window hash at the cut does not match, so a
            walk that took a window position from F1's candidates would miss the cut
  center    center-2 .. center+2: the last mask_s and the first mask_l position (first_cand's two
            ranges, W's switch), with the parity of eS
  max       max-2 .. max: the last tested position, the first untested one, the forced cut
  mid       cuts that come purely from the candidate lists
  phases    the chunk start's arena position mod 128 puts cs+a0, cs+a0+47, cs+center and the cut on
            the first and the last byte of a 128-byte line (load16_file's three loads, F1's LDS-DMA
            lines, 16-byte candidate groups straddling a line)
  tail      items that end t bytes after a chunk start (rem = t: `rem <= min`, center = rem < avg,
            the parity rule q < 2*(rem/2), rem = max +- 2) with matches planted at t-3 .. t-1
  position  cuts at k*sec + d, k*unit + d and 16*g + d' (section ends: F2/F3's entry of the next
            section, W's lane hand-over; unit ends: first_cand moving to the next unit's list; group
            ends), runs of max-sized chunks whose starts are the last / first byte of every section
  decoys    (a) a position in [a0+47, center) that clears mask_l but not mask_s, (b) a full-window
            match in the never-hashed first a0 bytes, (c) a position in the truncated window whose
            full-window hash matches while the hash started from 0 at a0 does not. F1 records all
            three as candidates; no walk may cut there.
  filler    "random" leaves many F1 candidates (shared bits clear) and no match; "zero" leaves none
            but the planted ones.

Only numpy and oracle.fastcdc are used; the product is never imported.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field

import numpy as np

from oracle import fastcdc as F

GEAR = np.array(F.gear_table(), dtype=np.uint64)
ANY = np.uint64(F.M64)  # an intermediate position with no condition (solve)
HASH_SPAN = 47  # positions from a0 whose window is truncated (kHashSpan in fastcdc_device.hpp)

CONFIGS = [
    (4096, 8192, 16384),
    (4096, 65536, 131072),
    (4096, 4096, 8192),
    (64, 256, 1024),
    (300, 257, 1500),
    (4096, 4120, 8192),    # the mask switch falls inside the truncated window
    (4097, 8191, 16383),   # odd min and max: the parity rule
]
WALK_CONFIGS = [CONFIGS[0], CONFIGS[2], CONFIGS[5], CONFIGS[6]]  # masks at bit 16 or above


def cfg_id(cfg) -> str:
    return "-".join(map(str, cfg))


# ------------------------------------------------------------------------------ hashes
def _roll64(g: np.ndarray) -> np.ndarray:
    """h[p] = sum_k g[p-k] << k over k = 0..63 (zeros before the array): six doubling steps."""
    h = g.astype(np.uint64, copy=True)
    w = 1
    while w < 64 and w < len(h):
        h[w:] += h[:-w] << np.uint64(w)
        w *= 2
    return h


def roll(data, a0: int = 0) -> np.ndarray:
    """The hash cut_gear holds after each of data[a0:], started from 0 at a0 (exact in all 64 bits):
    entry k belongs to position a0 + k."""
    return _roll64(GEAR[np.asarray(data, dtype=np.uint8)[a0:]])


def full(data, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """The full-window hash F1 sees at positions lo .. hi-1 of data: the 64 bytes up to and including
    the position (zeros before the array's start), which equals the 48-byte window in the bits below 48
    -- all a mask can test."""
    d = np.asarray(data, dtype=np.uint8)
    hi = len(d) if hi is None else hi
    s = max(0, lo - 63)
    return _roll64(GEAR[d[s:hi]])[lo - s:]


def geometry(cfg, rem: int):
    """(a0, eS, eL) of a chunk with `rem` bytes left in its file (rem > min)."""
    mn, av, mx = cfg
    center = av
    if rem > mx:
        rem = mx
    elif rem < center:
        center = rem
    return (mn // 2) * 2, (center // 2) * 2, (rem // 2) * 2


def mask_at(cfg, level: int, q):
    """The mask cut_gear applies at position q of a chunk with more than `max` bytes left."""
    ms, ml = F.masks(cfg[1], level)
    _, eS, _ = geometry(cfg, cfg[2] + 1)
    if np.isscalar(q):
        return ms if q < eS else ml
    return np.where(np.asarray(q) < eS, np.uint64(ms), np.uint64(ml))


# ------------------------------------------------------------------------------ the plan
@dataclass
class Cut:
    """One planned chunk: `L` bytes long, or (at) ending at absolute file position `at`, reached through
    filler chunks the generator solves for. decoys: a subset of "abc"; a_at: decoy (a)'s position in
    the chunk where the default will not do."""
    L: int | None = None
    at: int | None = None
    label: str = ""
    decoys: str = ""
    a_at: int | None = None


@dataclass
class Random:
    """Plain random bytes up to at least file position `until`; planting goes on at the oracle's next
    chunk start at or after it."""
    until: int


@dataclass
class Planted:
    data: np.ndarray
    lens: list            # promised chunk lengths, the whole file
    starts: list          # their starts
    labels: list          # the planner's label of each chunk
    decoys: list = field(default_factory=list)   # (kind, absolute position, chunk start)
    absent: list = field(default_factory=list)   # (label, L, why)
    hidden: list = field(default_factory=list)   # (cut, chunk start): truncated-window cuts no full-window hash shows

    def __iter__(self):  # data, lens = plant(...)
        return iter((self.data, self.lens))

    def label_at(self, start: int) -> str:
        i = int(np.searchsorted(np.asarray(self.starts), start, side="right")) - 1
        if i < 0:
            return "?"
        return self.labels[i] if self.starts[i] == start else f"inside {self.labels[i]!r} (+{start - self.starts[i]})"


class Planter:
    """Plants chunk after chunk at `pos` (plant() drives it from a plan; the lattices below drive it
    directly where the next entry depends on where the last one ended)."""

    def __init__(self, cfg, level, seed, filler="random"):
        self.cfg, self.level = cfg, level
        self.mn, self.av, self.mx = cfg
        self.ms, self.ml = (np.uint64(m) for m in F.masks(cfg[1], level))
        self.a0, self.eS, self.eL = geometry(cfg, cfg[2] + 1)
        self.lo = self.a0 + 3           # the shortest length a trigger search always reaches
        self.hi = self.eL - 1           # the longest length cut_gear can cut at before max
        self.rng = np.random.default_rng(seed)
        self.filler = filler
        self.buf = np.zeros(0, dtype=np.uint8)
        self.out = Planted(self.buf, [], [], [])
        self.pos = 0

    # -- storage
    def need(self, n: int):
        if n > len(self.buf):
            m = max(n, 2 * len(self.buf), 1 << 16)
            ext = self.rng.integers(0, 256, m - len(self.buf), dtype=np.uint8) if self.filler == "random" else \
                np.zeros(m - len(self.buf), dtype=np.uint8)
            self.buf = np.concatenate([self.buf, ext])

    def emit(self, L: int, label: str):
        self.out.starts.append(self.pos)
        self.out.lens.append(int(L))
        self.out.labels.append(label)
        self.pos += int(L)

    def masks(self, q0: int, q1: int) -> np.ndarray:
        return np.where(np.arange(q0, q1) < self.eS, self.ms, self.ml)

    # -- clean: no tested position in [q0, q1) of the chunk at cs may match
    def clean(self, cs: int, q0: int, q1: int):
        a0, buf = self.a0, self.buf
        if q1 <= q0:
            return
        mk = self.masks(q0, q1)
        bad = (roll(buf[cs:cs + q1], a0)[q0 - a0:] & mk) == 0
        cur = q0
        while True:
            idx = np.flatnonzero(bad[cur - q0:])
            if not len(idx):
                return
            # the first match: a value of its own byte with which it does not match (earlier positions do
            # not see that byte); the byte reaches the hashes of m .. m+63, which are tested again
            m = cur + int(idx[0])
            s, end = max(a0, m - 65), min(q1, m + 64)
            hprev = roll(buf[cs + s:cs + m])[-1:] if m > a0 else np.zeros(1, dtype=np.uint64)
            ok = np.flatnonzero((((hprev << np.uint64(1)) + GEAR) & mk[m - q0]) != 0)
            buf[cs + m] = ok[self.rng.integers(0, len(ok))]
            bad[m - q0:end - q0] = (roll(buf[cs + s:cs + end])[m - s:] & mk[m - q0:end - q0]) == 0
            assert not bad[m - q0]
            cur = m + 1

    # -- search the bytes at positions q-nb+1 .. q (nb <= 3) for: intermediate hashes that do not match
    # `mids`, post(final) & want == 0 and (veto) post(final) & veto != 0
    def solve(self, hprev: int, nb: int, mids, want, veto=None, post=None):
        G, one = GEAR, np.uint64(1)
        hp = np.array([hprev], dtype=np.uint64)  # (arrays wrap silently; numpy scalars warn)
        order = self.rng.permutation(256)
        found = []
        firsts = order if nb == 3 else [None]
        for b0 in firsts:
            if nb == 3:
                h1 = (hp << one) + G[b0:b0 + 1]
                if h1[0] & mids[0] == 0:
                    continue
                base, rest = h1, mids[1:]
            else:
                base, rest = hp, mids
            ok = np.ones(1, dtype=bool)
            for k in range(min(nb, 2)):
                base = ((base[:, None] << one) + G[None, :]).ravel()
                ok = np.repeat(ok, 256)
                if k < min(nb, 2) - 1:
                    ok &= (base & rest[k]) != 0
            fin = base if post is None else post(base)
            good = ok & ((fin & want) == 0)
            if veto is not None:
                good &= (fin & veto) != 0
            idx = np.nonzero(good)[0]
            if len(idx):
                i = int(idx[0])
                tail = [i] if nb == 1 else [i >> 8, i & 255]
                found = ([int(b0)] if nb == 3 else []) + tail
                break
        return found or None

    def trigger(self, cs: int, L: int) -> bool:
        """Make position L of the chunk at cs match its mask (bytes L-2 .. L, as many as are hashed)."""
        a0, buf = self.a0, self.buf
        nb = min(3, L - a0 + 1)
        q = L - nb  # the last position whose hash stays
        hprev = int(roll(buf[cs + max(a0, q - 64):cs + q + 1])[-1]) if q >= a0 else 0
        mids = [mask_at(self.cfg, self.level, p) for p in range(L - nb + 1, L)]
        got = self.solve(hprev, nb, [np.uint64(m) for m in mids], np.uint64(mask_at(self.cfg, self.level, L)))
        if got is None:
            return False
        buf[cs + L - nb + 1:cs + L + 1] = got
        return True

    # -- decoys
    def decoy_b(self, cs: int):
        q = max(8, self.a0 // 2)
        if q + 8 > self.a0 - 3:
            return
        hprev = int(full(self.buf, cs + q - 3, cs + q - 2)[0])
        got = self.solve(hprev, 3, [ANY, ANY], self.ms)
        if got:
            self.buf[cs + q - 2:cs + q + 1] = got
            self.out.decoys.append(("b", cs + q, cs))

    def decoy_c(self, cs: int, L: int):
        a0 = self.a0
        q = a0 + 4
        if L < q + 4 or a0 < 16:
            return
        k = np.uint64(q - a0 + 1)
        t = roll(self.buf[cs:cs + q + 1], a0)[-1]
        hprev = int(full(self.buf, cs + a0 - 4, cs + a0 - 3)[0])
        want = np.uint64(mask_at(self.cfg, self.level, q))
        got = self.solve(hprev, 3, [ANY, ANY], want, post=lambda h: t + (h << k))
        if got:
            self.buf[cs + a0 - 3:cs + a0] = got
            self.out.decoys.append(("c", cs + q, cs))

    def decoy_a(self, cs: int, L: int, q: int | None = None):
        a0 = self.a0
        q = a0 + HASH_SPAN + 17 if q is None else q
        if q >= self.eS or q > L - 3 or q < a0 + HASH_SPAN:
            return None
        hprev = int(roll(self.buf[cs + max(a0, q - 67):cs + q - 2])[-1])
        got = self.solve(hprev, 3, [self.ms, self.ms], self.ml, veto=self.ms)
        if got:
            self.buf[cs + q - 2:cs + q + 1] = got
            self.out.decoys.append(("a", cs + q, cs))
            return q
        return None

    # -- one chunk of L bytes at self.pos
    def chunk(self, L: int, label: str, decoys: str = "", a_at: int | None = None):
        cs, a0 = self.pos, self.a0
        assert a0 <= L <= self.mx, (label, L)
        self.need(cs + self.mx + 64)
        forced = L >= self.eL
        end = self.eL if forced else L
        if "b" in decoys:
            self.decoy_b(cs)
        self.clean(cs, a0, end)
        if "c" in decoys:
            self.decoy_c(cs, L)
        if "a" in decoys:
            q = self.decoy_a(cs, end, a_at)
            if q is not None:
                self.clean(cs, q + 1, end)
        if forced:
            if L != self.mx:
                self.out.absent.append((label, L, "never tested (q >= eL)"))
            self.emit(self.mx, label)
            return
        if not self.trigger(cs, L):
            assert L - a0 <= 2, (label, L, "no trigger found")
            self.out.absent.append((label, L, f"no value of the {L - a0 + 1} hashed byte(s) matches"))
            # nothing planted: the chunk is whatever the cleaned bytes after it give; plan a forced one
            self.clean(cs, L, self.eL)
            self.emit(self.mx, label)
            return
        if L - a0 < HASH_SPAN and "c" not in decoys:
            # a cut in the truncated window that the full-window hash does not show (at j = 46 the two
            # differ in bit 47 alone, by the low bit of GEAR[byte a0-1]): only the walks' own hash of the
            # bytes from a0 finds it, never F1's candidates
            mask = np.uint64(mask_at(self.cfg, self.level, L))
            for b in self.rng.permutation(256):
                self.buf[cs + a0 - 1] = b
                if full(self.buf, cs + L, cs + L + 1)[0] & mask != 0:
                    self.out.hidden.append((cs + L, cs))
                    break
        self.emit(L, label)

    def fill_to(self, at: int, label: str, decoys: str, fill: int):
        """Filler chunks, then one chunk that ends at absolute position `at`."""
        lo, hi = self.lo, self.hi
        while True:
            d = at - self.pos
            if lo <= d <= hi:
                self.chunk(d, label, decoys)
                return
            assert d >= 2 * lo, (label, at, self.pos, "anchors too close")
            # a filler after which the rest is one plantable chunk, or long enough for two
            first = max(lo, min(fill, hi))
            f = next((f for f in itertools.chain(range(first, hi + 1), range(lo, first))
                      if lo <= d - f <= hi or d - f >= 2 * lo), None)
            assert f is not None, (label, at, self.pos)
            self.chunk(f, "fill")

    def random_until(self, until: int):
        if until <= self.pos:
            return
        n = until + 2 * self.mx + 1
        self.need(n)
        if self.filler != "random":
            self.buf[self.pos:n] = self.rng.integers(0, 256, n - self.pos, dtype=np.uint8)
        ch = F.chunks(self.buf[self.pos:n], self.mn, self.av, self.mx, self.level)
        for o, ln in ch.tolist():
            if self.pos >= until:
                break
            assert self.pos + ln + self.mx < n
            self.emit(ln, "random")


    def add(self, e, fill: int | None = None):
        """One plan entry: an int (a length), a Cut or a Random."""
        fill = fill if fill is not None else self.a0 + max(64, (self.eS - self.a0) // 2)
        if isinstance(e, Random):
            self.random_until(e.until)
            return
        if not isinstance(e, Cut):
            e = Cut(L=int(e), label=f"L={int(e)}")
        if e.at is not None:
            self.fill_to(e.at, e.label, e.decoys, fill)
        else:
            self.chunk(e.L, e.label, e.decoys, e.a_at)

    def finish(self, tail: int | None = None) -> Planted:
        """A forced max-sized guard chunk (so that every planned chunk had more than `max` bytes left
        and cut_gear's center and eL were the interior ones), then `tail` <= min bytes: one last chunk."""
        self.chunk(self.mx, "guard")
        tail = min(self.mn, 17) if tail is None else tail
        assert 0 <= tail <= self.mn
        self.need(self.pos + tail)
        if tail:
            self.emit(tail, "tail")
        self.out.data = self.buf[:self.pos].copy()
        return self.out


def plant(cfg, level, plan, seed, filler: str = "random", prefix: int = 0, tail: int | None = None,
          fill: int | None = None, size_hint: int = 0) -> Planted:
    """A byte array and the chunk lengths it promises (Planted unpacks to the two). plan: ints, Cut and
    Random entries; prefix: random bytes first (planting starts at the oracle's next chunk start);
    tail: bytes after the guard chunk that follows the last planned one (at most min: one last chunk);
    fill: the length filler chunks before an anchored cut aim for; size_hint: the expected file size
    (one allocation)."""
    p = Planter(cfg, level, seed, filler)
    p.need(size_hint)
    if prefix:
        p.random_until(prefix)
    for e in plan:
        p.add(e, fill)
    return p.finish(tail)


# ------------------------------------------------------------------------------ the lattices
def line_phases(cfg):
    """Chunk-start phases (arena position mod 128) that put cs+a0, cs+a0+47 and cs+center on the first
    and on the last byte of a 128-byte line, with their names."""
    a0, eS, _ = geometry(cfg, cfg[2] + 1)
    out = []
    for name, x in (("a0", a0), ("a0+47", a0 + HASH_SPAN), ("center", cfg[1])):
        out += [(f"{name}@first", (-x) % 128), (f"{name}@last", (127 - x) % 128)]
    return out


def length_classes(cfg):
    """[(class, label, L)] of the length lattice."""
    mn, av, mx = cfg
    a0, eS, eL = geometry(cfg, mx + 1)
    out = [("trunc", f"trunc j={j}", a0 + j) for j in range(50)]
    out += [("center", f"center{d:+d}", av + d) for d in range(-2, 3) if a0 <= av + d <= mx]
    out += [("max", f"max{d:+d}" if d else "max", mx + d) for d in (-2, -1, 0)]
    lo_mid = a0 + HASH_SPAN + 100
    mids = sorted({max(lo_mid, (a0 + max(av, a0 + 200)) // 2 + 1), (max(av, a0) + mx) // 2 + 1})
    out += [("mid", f"mid L={L}", L) for L in mids]
    return out


ITEM_PHASES = (0, 1, 15, 16, 64, 127)


@dataclass
class Lattice:
    planted: Planted
    offs: np.ndarray
    lens: np.ndarray
    names: list
    coverage: dict


def _phase_fill(p_lo, pos, phase):
    """A filler length >= p_lo after which the next chunk starts at `phase` mod 128."""
    return p_lo + (phase - pos - p_lo) % 128


def length_lattice(cfg, level: int = 1, filler: str = "random", seed: int = 1) -> Lattice:
    """Every class length twice -- once plain with the cut on the last byte of a line, once with decoys
    at a phase from line_phases (cycled; the cut on the first byte of a line for the long classes) -- in
    one chain, cut into six items that start at ITEM_PHASES past a 128-byte boundary, plus the whole
    chain as one item."""
    a0, eS, eL = geometry(cfg, cfg[2] + 1)
    classes = length_classes(cfg)
    phases = line_phases(cfg)
    p = Planter(cfg, level, seed, filler)
    cov, starts = {}, []
    per_item = (2 * len(classes) + 5) // 6

    def hit(cls, cs, L):
        ev = cov.setdefault(cls, set())
        for name, x in (("a0", a0), ("a0+47", a0 + HASH_SPAN), ("center", cfg[1]), ("cut", L)):
            if (cs + x) % 128 == 0:
                ev.add(f"{name}@first")
            if (cs + x) % 128 == 127:
                ev.add(f"{name}@last")

    k = 0
    for rep in range(2):
        for i, (cls, label, L) in enumerate(classes):
            if k % per_item == 0 and len(starts) < 6:
                if starts:
                    p.chunk(_phase_fill(p.lo, p.pos, ITEM_PHASES[len(starts)]), "fill item-phase")
                starts.append(p.pos)
            real = cfg[2] if L >= eL else L
            if rep == 0:
                ph = (127 - real) % 128
            elif cls == "trunc":
                ph = phases[i % len(phases)][1]
            else:
                ph = (-real) % 128 if i % 2 else phases[4 + (i // 2) % 2][1]
            p.chunk(_phase_fill(p.lo, p.pos, ph), "fill phase")
            cs = p.pos
            p.chunk(L, label + (" +decoys" if rep else ""), "abc" if rep else "")
            if p.out.lens[-1] == real:  # (not an absent length)
                hit(cls, cs, real)
                cov[cls].add("decoys" if rep else "plain")
            k += 1
    pl = p.finish(tail=cfg[0])
    assert [s % 128 for s in starts] == list(ITEM_PHASES), [s % 128 for s in starts]
    ends = starts[1:] + [pl.starts[-2]]  # (the guard chunk's start)
    # an item ends min/2 bytes into the next item's first chunk: one last chunk of <= min bytes
    offs = [0] + starts
    lens = [len(pl.data)] + [e + cfg[0] // 2 - s for s, e in zip(starts, ends)]
    names = ["whole"] + [f"phase {ph}" for ph in ITEM_PHASES]
    for kind in "abc":
        cov.setdefault("decoy", set())
        if any(d[0] == kind for d in pl.decoys):
            cov["decoy"].add(kind)
    cov = {c: sorted(v) for c, v in cov.items()}
    return Lattice(pl, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64), names, cov)


def tail_lengths(cfg):
    mn, av, mx = cfg
    t = set(range(mn - 1, mn + 51)) | set(range(av - 2, av + 3)) | set(range(mx - 2, mx + 3))
    return sorted(x for x in t if x > 0)


def tail_lattice(cfg, level: int = 1, seed: int = 2) -> Lattice:
    """Items that end t bytes after a chunk start, t in tail_lengths(cfg), with a match planted at
    t-1, t-2 or t-3: a chain of chunks of every plantable length L in {t-3, t-2, t-1}; the item of (L, t)
    starts at the chunk before the one of length L and ends t bytes into it."""
    a0, eS, eL = geometry(cfg, cfg[2] + 1)
    ts = tail_lengths(cfg)
    Ls = sorted({t - k for t in ts for k in (1, 2, 3) if a0 <= t - k < eL})
    plan = [Cut(L=a0 + 64, label="lead")] + [Cut(L=L, label=f"tail L={L}") for L in Ls]
    plan.append(Cut(L=cfg[2], label="tail forced"))  # for the t no planted match can sit before
    pl = plant(cfg, level, plan, seed, tail=cfg[0])
    first = {ln_label: i for i, ln_label in enumerate(pl.labels)}
    offs, lens, names, cov = [], [], [], {"t<=min": 0, "odd t, match at t-1": 0, "even t, match at t-1": 0,
                                          "center=rem<avg": 0, "t>max": 0, "t==max": 0}
    n = len(pl.data)
    for L in Ls:
        i = first.get(f"tail L={L}")
        if i is None or pl.lens[i] != L:
            continue  # an absent length (reported by the planter)
        cs, prev = pl.starts[i], pl.starts[i - 1]
        for t in ts:
            if not (L + 1 <= t <= L + 3) or cs + t > n:
                continue
            offs.append(prev)
            lens.append(cs + t - prev)
            names.append(f"t={t} match at t-{t - L}")
            cov["odd t, match at t-1"] += t % 2 == 1 and t - L == 1
            cov["even t, match at t-1"] += t % 2 == 0 and t - L == 1
            cov["center=rem<avg"] += cfg[0] < t < cfg[1]
            cov["t>max"] += t > cfg[2]
            cov["t==max"] += t == cfg[2]
    # t <= min has no tested position: items that end there after any chunk start; and a t without a
    # plantable length in t-3 .. t-1 (an absent one, or past eL when max is odd) ends in the forced chunk
    done = {int(nm.split()[0][2:]) for nm in names}
    i = pl.labels.index("tail forced")
    for t in ts:
        if t not in done and t > cfg[0] + 3:
            offs.append(pl.starts[i - 1])
            lens.append(pl.starts[i] + t - pl.starts[i - 1])
            names.append(f"t={t} no match")
            cov["t>max"] += t > cfg[2]
    cs, prev = pl.starts[2], pl.starts[1]
    for t in ts:
        if t <= cfg[0] + 3:
            offs.append(prev)
            lens.append(cs + t - prev)
            names.append(f"t={t} short")
            cov["t<=min"] += t <= cfg[0]
    return Lattice(pl, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64), names, cov)


D_OFFSETS = (-49, -48, -47, -17, -16, -15, -1, 0, 1, 15, 16, 17, 47, 48, 49)
# the same, the window offsets first: what a file with room for fewer anchors keeps
D_BY_WEIGHT = (-49, -48, -47, 47, 48, 49, 0, -1, 1, -17, -16, -15, 15, 16, 17)
AFTER_STORED = (5, 21)  # byte in its unit of the stored candidate (decoy a) and of the cut in the next group


def min_section(cfg) -> int:
    """The smallest section oxh_fastcdc_device accepts: max rounded up to 8 KiB."""
    return (cfg[2] + 8191) // 8192 * 8192


def position_lattice(cfg, sec: int, level: int = 1, seed: int = 3, runs: bool = True) -> Lattice:
    """One file (one item at arena offset 0) with cuts anchored at k*sec + d and k*unit + d for d in
    D_OFFSETS, at 16*g + 0 and 16*g + 15, one right after a unit's first candidate group (with
    OXH_CDC_UNIT_CAP=1 the first group past the stored list), and -- runs, for sec == max -- two runs of
    nine forced max-sized chunks whose starts are the last and then the first byte of consecutive
    sections."""
    a0, eS, eL = geometry(cfg, cfg[2] + 1)
    mx, unit, lo = cfg[2], sec // 64, a0 + 3
    gap = ((2 * lo + 200 + sec - 1) // sec) * sec  # whole sections, room for two chunks between anchors
    plan, cov, at = [], {}, 0
    for i, d in enumerate(D_OFFSETS):
        at = (i + 1) * gap + d
        plan.append(Cut(at=at, label=f"sec k={(i + 1) * gap // sec} d={d:+d}"))
        cov["section"] = cov.get("section", 0) + 1
    ugap = 2 * lo + 300  # room for two chunks between anchors, whatever their offsets
    for d in D_OFFSETS:
        k = (at + ugap) // unit + 1
        if k % 64 == 0:  # keep the unit anchors off the section boundaries
            k += 1
        at = k * unit + d
        plan.append(Cut(at=at, label=f"unit k={k} d={d:+d}"))
        cov["unit"] = cov.get("unit", 0) + 1
    for dd in (0, 15):
        g = (at + ugap) // 16 + 3
        at = 16 * g + dd
        plan.append(Cut(at=at, label=f"group g={g} d'={dd}"))
        cov["group"] = cov.get("group", 0) + 1
    # a cut in the group right after a unit's stored candidate (OXH_CDC_UNIT_CAP=1: one group per unit):
    # decoy (a) -- a candidate, mask_l clear -- at byte AFTER_STORED[0] of a unit, in its first group (so no
    # group of the unit comes before it, whatever the filler holds), the cut 16 bytes on in the second
    qd = a0 + HASH_SPAN + 17
    if qd + 16 < eS:
        u0 = ((at + 2 * lo + 300 + qd) // unit + 1) * unit
        plan.append(Cut(at=u0 + AFTER_STORED[0] - qd, label="lead to after-stored"))
        plan.append(Cut(L=qd + 16, label="cut in the group after a stored candidate", decoys="a", a_at=qd))
        cov["after-stored-candidate"] = 1
        at = u0 + AFTER_STORED[1]
    if runs and sec == mx:
        for name, ph in (("last", sec - 1), ("first", 0)):
            k = (at + 2 * lo + 200) // sec + 1
            plan.append(Cut(at=k * sec + ph, label=f"run-{name} lead"))
            for r in range(9):
                plan.append(Cut(L=mx, label=f"run-{name} {r}"))
            at = k * sec + ph + 9 * mx
            cov[f"run-{name}"] = 9
    pl = plant(cfg, level, plan, seed, tail=min(cfg[0], 33))
    return Lattice(pl, np.array([0], dtype=np.uint64), np.array([len(pl.data)], dtype=np.uint64), ["file"], cov)


def default_sections(cfg, path: str) -> int:
    """The section size oxh_fastcdc_device derives for a small input (its sizing loop): the scan takes
    max(512 KiB, 8 * max), the walk max(64 KiB, 4 * max), max rounded up to 1 KiB, whole 8 KiB."""
    mr = (cfg[2] + 1023) // 1024 * 1024
    s = max(512 * 1024, 8 * mr) if path == "scan" else max(64 * 1024, 4 * mr)
    return (s + 8191) // 8192 * 8192


DEFAULT_CASES = [(CONFIGS[0], "scan"), (CONFIGS[0], "walk"), (CONFIGS[1], "scan")]  # (cfg, path) run without override


def default_lattice(cfg, path: str, level: int = 1, seed: int = 4) -> Lattice:
    """Cuts anchored around the default plan's section boundaries (no section override): one offset of
    D_OFFSETS per boundary, as many boundaries as a file under 8 MiB has (the last anchor, the guard chunk
    and the tail fit), the offsets in D_BY_WEIGHT's order where that is fewer than all."""
    sec = default_sections(cfg, path)
    n = min(len(D_OFFSETS), ((8 << 20) - 49 - cfg[2] - cfg[0] - 1) // sec)
    ds = D_BY_WEIGHT[:n]
    plan = [Cut(at=(i + 1) * sec + d, label=f"default-sec k={i + 1} d={d:+d}") for i, d in enumerate(ds)]
    pl = plant(cfg, level, plan, seed, fill=(cfg[1] + cfg[2]) // 2)
    assert len(pl.data) < 8 << 20
    return Lattice(pl, np.array([0], dtype=np.uint64), np.array([len(pl.data)], dtype=np.uint64), ["file"],
                   {"default-section": len(ds)})


EDGE_CASES = (
    "chunk starts at E-max, forced max: every chunk final, carry = E",
    "chunk starts at E-max, short: the next start is carried; a planted cut ends at E",
    "chunk starts at E-max+1 (carried), planted cut at E-1; a chunk starts at E-1",
    "chunk starts at E-max-1, short; a planted cut ends at E+1",
    "truncated window straddles E, cut planted before E",
    "truncated window straddles E, cut planted after E",
    "chunk starts at E-max+1 (carried), planted cut ends at E",
    "chunk starts at E-max-1, forced max ends at E-1; a chunk starts at E-1",
)


def edge_plan(cfg, E: int, case: int):
    """The plan entries that put EDGE_CASES[case] at segment end E of the host pipeline (stitch() in
    fastcdc_host.cpp: a chunk at pos is carried when pos + max > E, kept when pos + max == E)."""
    mn, av, mx = cfg
    a0, eS, eL = geometry(cfg, mx + 1)
    name = f"E={E} case {case}: "
    lead = [Random(until=E - 4 * mx)]
    if case == 0:
        return lead + [Cut(at=E - mx, label=name + "lead"), Cut(L=mx, label=name + "forced max from E-max"),
                       Cut(L=a0 + 100, label=name + "starts at E")]
    if case == 1:
        return lead + [Cut(at=E - mx, label=name + "lead"), Cut(L=a0 + 100, label=name + "short from E-max"),
                       Cut(at=E, label=name + "planted cut ends at E")]
    if case == 2:
        return lead + [Cut(at=E - mx + 1, label=name + "lead"), Cut(at=E - 1, label=name + "planted cut at E-1"),
                       Cut(L=a0 + 60, label=name + "starts at E-1")]
    if case == 3:
        return lead + [Cut(at=E - mx - 1, label=name + "lead"), Cut(L=a0 + 200, label=name + "short from E-max-1"),
                       Cut(at=E + 1, label=name + "planted cut ends at E+1")]
    if case in (4, 5):
        return lead + [Cut(at=E - a0 - 23, label=name + "lead"),
                       Cut(L=a0 + (10 if case == 4 else 40), label=name + "window straddles E")]
    if case == 6:
        return lead + [Cut(at=E - mx + 1, label=name + "lead"), Cut(at=E, label=name + "planted cut ends at E")]
    if case == 7:
        return lead + [Cut(at=E - mx - 1, label=name + "lead"), Cut(L=mx, label=name + "forced max ends at E-1"),
                       Cut(L=a0 + 80, label=name + "starts at E-1")]
    raise ValueError(case)


def edge_file(cfg, ends, cases, size: int, seed: int, level: int = 1) -> Planted:
    """A random file of about `size` bytes with edge_plan(cases[i]) planted at ends[i]."""
    plan = []
    for E, c in zip(ends, cases):
        plan += edge_plan(cfg, E, c)
    plan.append(Random(until=size))
    return plant(cfg, level, plan, seed, size_hint=size + 4 * cfg[2])


def explain(pl: Planted, item_off: int, want: np.ndarray, got_off, got_len) -> str:
    """The first chunk of an item where the device and the oracle part: the planner's label of the chunk
    that starts there, its start in the planted file, the expected and the actual length."""
    n = min(len(want), len(got_off))
    for k in range(n):
        if int(got_off[k]) != int(want[k, 0]) or int(got_len[k]) != int(want[k, 1]):
            break
    else:
        k = n
    if k >= len(want):
        return f"{len(got_off)} chunks, expected {len(want)} (extra chunks at the end)"
    start = item_off + int(want[k, 0])
    act = int(got_len[k]) if k < len(got_off) and int(got_off[k]) == int(want[k, 0]) else None
    return (f"chunk {k}: class {pl.label_at(start)!r}, start {start} (item +{int(want[k, 0])}), "
            f"expected length {int(want[k, 1])}, actual {act}")
