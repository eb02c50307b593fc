"""The case families of the CSV float conversions (tests/test_csv_floats_cpu.py pins them and the host build of the
headers, tests/test_csv_floats.py sends the same cells through the GPU). Plain Python and numpy with seeded
generators; nothing of the library and neither restatement is imported here: a reader family is a list of texts
(bytes), a writer family a list of doubles, and what each cell must give comes from tests/_csv.py and
tests/_csvwrite.py where the cells are used.

Reader families: R1 decimal-born texts of every digit count and exponent in every shape of the grammar, R2 the
boundary of the exact path (m around 2^53, the u64's 19 and 20 digits; e10 around +-22), R3 the ties of the one
multiplication, R4 the exponent clamp and the zeros, R5 texts that are not the grammar.
Writer families: W1 decimal-born doubles of every digit count and decimal exponent, W2 the 15-digit integers around
1e15 at every scale, W3 the powers of two and of ten with their neighbours, W4 random bits.
Each family comes as generated (nearly wave-uniform in the power of ten or in ryu's form) and shuffled with a fixed
seed (every wave mixes them, and the deferred cells)."""
import random
import struct

import numpy as np

SEED = 20261021


# ---------------------------------------------------------------- reader
def shapes(m: str, e: int) -> list:
    """The decimal m x 10^e (m: digits, the first one not zero) in every shape of the grammar."""
    L = len(m)
    out = [f"{m}e{e}", f"{m}E{e:+d}", f"+{m}e{e}", f"-000{m}.e{e}"]
    for p in sorted({1, L // 2, L}):                       # the point after p digits: 0 is ".ddd"
        out.append(f"{m[:p]}.{m[p:]}e{e + L - p}")
    if 0 <= e <= 25:
        out.append(m + "0" * e)                            # the zeros are significant digits: past 19 of them, deferred
    if -40 <= e < 0:
        out.append(f"{m[:L + e]}.{m[L + e:]}" if L + e > 0 else "0." + "0" * -(L + e) + m)
    return [s.encode() for s in out]


def r1(reps: int = 3) -> list:
    rng = random.Random(SEED + 1)
    out = []
    for L in range(1, 21):
        for e in range(-25, 26):
            for _ in range(reps):
                out += shapes(str(rng.randrange(10 ** (L - 1), 10 ** L)), e)
    return out


R2_MANTISSAS = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 10 ** 19 - 1, 10 ** 19, 2 ** 64 - 1, 2 ** 64, 10 ** 18, 10 ** 15]
R2_EXPONENTS = [-24, -23, -22, -21, -1, 0, 1, 21, 22, 23, 24]


def r2() -> list:
    return [s for m in R2_MANTISSAS for e in R2_EXPONENTS for s in shapes(str(m), e)]


def r3_pairs(per: int = 40) -> list:
    """(m, j): odd m <= 2^53 with 2^53 <= m 5^j < 2^54, so that m 10^j = (m 5^j) 2^j needs 54 bits and lies halfway
    between two doubles. `per` of them for each j in 1..22, evenly over the range, or all there are."""
    out = []
    for j in range(1, 23):
        lo, hi = -(-2 ** 53 // 5 ** j), min((2 ** 54 - 1) // 5 ** j, 2 ** 53)
        lo += 1 - lo % 2                                   # the first odd one
        count = (hi - lo) // 2 + 1
        picks = range(count) if count <= per else sorted({(count - 1) * i // (per - 1) for i in range(per)})
        out += [(lo + 2 * i, j) for i in picks]
    return out


def r3() -> list:
    return [b"%de%d" % pair for pair in r3_pairs()]


def r4() -> list:
    return [b"1e100000", b"1e100001", b"1e-100001", b"0e99999999999", b"0.0e-999999", b"1e4294967297",
            b"1e+0000000000000000000000000022", b"1e-0000000000000000000000022", b"0" * 24 + b"1",
            b"0.0000000000000000000001", b"0.00000000000000000000001"] + [b"1" + b"0" * z for z in (18, 19, 22, 23)]


R5 = [b"1e", b"1e+", b".", b"e5", b"1.5.2", b"0x10", b"1_000", b"1 ", b" 1", b"--1", b"infinit", b"nan0"]


def with_r5(texts: list, every: int = 64) -> list:
    """R5 among the values: one of its cells in front of every `every` - 1 texts, in turn."""
    out = []
    for k in range(0, len(texts), every - 1):
        out.append(R5[(k // (every - 1)) % len(R5)])
        out += texts[k:k + every - 1]
    return out


def shuffled(cells: list, seed: int = SEED) -> list:
    out = list(cells)
    random.Random(seed).shuffle(out)
    return out


def reader_families() -> dict:
    """name -> texts, every one the grammar; R5 goes in through with_r5."""
    return {"R1": r1(), "R2": r2(), "R3": r3(), "R4": r4()}


# ---------------------------------------------------------------- writer
def both_signs(values: list) -> list:
    return [s * v for v in values for s in (1.0, -1.0)]


def w1(reps: int = 40) -> list:
    rng = random.Random(SEED + 2)
    out = []
    for L in range(1, 18):
        for kk in range(-26, 27):
            for _ in range(reps):
                d = str(rng.randrange(1, 10)) if L == 1 else (
                    str(rng.randrange(1, 10)) + "".join(str(rng.randrange(10)) for _ in range(L - 2)) + str(rng.randrange(1, 10)))
                out.append(float(f"{d}e{kk - L}"))
    return both_signs(out)


W2_DIGITS = [999999999999999, 999999999999998, 100000000000001, 100000000000000, 99999999999999]


def w2() -> list:
    return both_signs([float(f"{d}e{k}") for d in W2_DIGITS for k in range(-37, 1)])


def from_bits(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def to_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def w3() -> list:
    """2^e (e = -1074 .. 1023) and 1e{e} (e = -323 .. 308), each with the double below and the one above it, and the
    double below 2^1024, the largest; the zero below 2^-1074 is left out (the zeros are no digits)."""
    out = []
    for centre in [2.0 ** e for e in range(-1074, 1024)] + [float("inf")] + [float(f"1e{e}") for e in range(-323, 309)]:
        b = to_bits(centre)
        out += [from_bits(n) for n in (b - 1, b, b + 1) if 0 < n < 0x7FF0000000000000]
    return both_signs(out)


def w4(n: int = 1 << 17) -> list:
    """Random bits, the non-finite ones replaced by 1.5, as repr_case() of tests/test_csv.py has them."""
    rng = np.random.default_rng(SEED % 1000)
    bits = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    bits[:64] &= np.uint64(0x800FFFFFFFFFFFFF)             # subnormals
    bits = np.where(np.isfinite(bits.view(np.float64)), bits, np.uint64(0x3FF8000000000000))
    return bits.view(np.float64).tolist()


def writer_families() -> dict:
    return {"W1": w1(), "W2": w2(), "W3": w3(), "W4": w4()}


# ---------------------------------------------------------------- integers
def integers() -> list:
    """Every digit count 1..19 at both of its ends, for both signs, and the two ends of int64."""
    out = []
    for k in range(19):
        out += [10 ** k - 1, -(10 ** k - 1), 10 ** k, -(10 ** k)]
    return out + [-(1 << 63), (1 << 63) - 1]
