"""The CSV float conversions without a GPU: the case families of tests/_floatcases.py are what they are meant to be
(counted from the restatements of tests/_csv.py and tests/_csvwrite.py alone, so that a changed generator cannot
quietly empty a case), and csv_number.hpp / csv_text.hpp -- the code the kernels run -- compiled for the host give the
restatements' answer on every cell: the value's bits or the text, and which cells are deferred
(tests/native/csv_float_cases.cpp). This is the leg that says "the rule is right"; tests/test_csv_floats.py sends the
same cells through the GPU and says "the device computes the rule". Its expectations are the functions below."""
import functools
import struct
import subprocess
from collections import Counter

import numpy as np

import _floatcases as F
from test_csv_write_cpu import C, W

SPECIAL_BITS = [0, 1 << 63, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF80000DEADBEEF, 0xFFF0000000000001, 0x7FF0000000000000,
                0xFFF0000000000000]   # the zeros, four NaNs, the infinities: no digits


# ---------------------------------------------------------------- what every cell must give (also the GPU leg's)
@functools.lru_cache(maxsize=None)
def reader_texts(name: str, order: str = "generated") -> tuple:
    """A family's texts in one of its two orders. "R5": its cells among the first of R1's; "all": R1 to R4; "all+R5"."""
    if order == "shuffled":
        return tuple(F.shuffled(reader_texts(name), seed=F.SEED + len(name)))
    families = F.reader_families()
    if name in families:
        return tuple(families[name])
    if name == "R5":
        return tuple(F.with_r5(families["R1"][:63 * len(F.R5)]))
    everything = [t for texts in families.values() for t in texts]
    return tuple(F.with_r5(everything) if name == "all+R5" else everything)


@functools.lru_cache(maxsize=None)
def read_cell(text: bytes):
    """None (a null), or (bits, deferred) by float() behind the grammar."""
    return C.parse_float(text)


def reader_want(texts) -> C.Buffers:
    """The FLOAT64 column of a one-cell-per-row file of these texts."""
    cells = [read_cell(t) for t in texts]
    n = len(cells)
    bits = np.array([0 if c is None else c[0] for c in cells], dtype=np.uint64)
    valid = np.array([c is not None for c in cells], dtype=bool)
    return C.Buffers(bits, None, C.pack(valid), (0, int(n - valid.sum()), sum(c[1] for c in cells if c is not None), 8 * n))


def mantissa_e10(text: bytes):
    """(m, e10) of a text of the grammar as the exact path sees it: the digits as an integer, the decimal exponent of
    the last one."""
    g = C.FLOAT_RE.fullmatch(text)
    whole, frac = g.group(2) or b"", (g.group(3) if g.group(2) is not None else g.group(4)) or b""
    return int(whole + frac), int(g.group(5) or 0) - len(frac)


@functools.lru_cache(maxsize=None)
def writer_values(name: str, order: str = "generated") -> tuple:
    if order == "shuffled":
        return tuple(F.shuffled(writer_values(name), seed=F.SEED + len(name) + ord(name[1])))
    return tuple({"W1": F.w1, "W2": F.w2, "W3": F.w3, "W4": F.w4}[name]())


@functools.lru_cache(maxsize=None)
def write_cell(bits: int):
    """(text, deferred) by repr() in ryu's forms."""
    x = F.from_bits(bits)
    return W.float_text(x), W.float_deferred(x)


def writer_want(values):
    """([text], [deferred]) of a column of doubles."""
    cells = [write_cell(F.to_bits(v)) for v in values]
    return [c[0] for c in cells], [c[1] for c in cells]


def layout(text: bytes) -> str:
    """Which of ryu's five forms a finite non-zero double's text has, by its look."""
    t = text.lstrip(b"-")
    if b"e" in t:
        return "d.ddde" if b"." in t else "de"
    return "0.00ddd" if t.startswith(b"0.") else "ddd00.0" if t.endswith(b".0") else "dd.dd"


# ---------------------------------------------------------------- the families
def test_the_writer_families_hold_what_they_are_for():
    exact_j, exact_L, layouts, deferred, sizes = Counter(), Counter(), Counter(), 0, {}
    for name in ("W1", "W2", "W3"):
        values = writer_values(name)
        texts, flags = writer_want(values)
        sizes[name] = (len(values), len(values) - sum(flags), sum(flags))
        for v, text, late in zip(values, texts, flags):
            layouts[layout(text)] += 1
            if late:
                deferred += 1
                continue
            d, k = W.float_digits(abs(v))
            exact_j[max(-k, 0)] += 1
            exact_L[len(d)] += 1
    exact = sum(exact_j.values())
    print("writer families (cells, exact, deferred):", sizes, "W4:", len(writer_values("W4")))
    print("exact", exact, "deferred", deferred, "per j min", min(exact_j[j] for j in range(23)), "per L min", min(exact_L[n] for n in range(1, 16)),
          "layouts", dict(layouts))
    assert exact >= 15000 and deferred >= 15000
    assert sorted(exact_j) == list(range(23)) and all(exact_j[j] >= 500 for j in range(23)), sorted(exact_j.items())
    assert sorted(exact_L) == list(range(1, 16)) and all(exact_L[n] >= 500 for n in range(1, 16)), sorted(exact_L.items())
    assert len(layouts) == 5 and all(count >= 3000 for count in layouts.values()), layouts
    assert sizes["W1"][0] == 2 * 17 * 53 * 40 and sizes["W2"][0] == 2 * 5 * 38 and sizes["W3"][0] == 2 * 3 * (2098 + 632)
    values = writer_values("W3")
    for landmark in (5e-324, W.MIN_NORMAL, F.from_bits(F.to_bits(W.MIN_NORMAL) - 1), 1.7976931348623157e308, 1e15, F.from_bits(F.to_bits(1e15) - 1),
                     1e-22, 1e22, 1e-323, 1e308):
        assert landmark in values and -landmark in values, landmark
    w4 = writer_values("W4")
    assert len(w4) == 1 << 17 and all(v == v and abs(v) != float("inf") for v in w4)
    assert sorted(writer_values("W1", "shuffled")) == sorted(writer_values("W1")) and writer_values("W1", "shuffled") != writer_values("W1")


def test_the_reader_families_hold_what_they_are_for():
    exact_e10, exact, deferred, sizes = Counter(), 0, 0, {}
    for name in ("R1", "R2", "R3", "R4"):
        texts = reader_texts(name)
        cells = [read_cell(t) for t in texts]
        assert None not in cells, (name, [t for t, c in zip(texts, cells) if c is None][:5])
        sizes[name] = (len(texts), sum(not c[1] for c in cells), sum(c[1] for c in cells))
        for t, (_, late) in zip(texts, cells):
            deferred += late
            exact += not late
            m, e10 = mantissa_e10(t)
            if not late and m:
                assert m <= 1 << 53 and abs(e10) <= 22
                exact_e10[e10] += 1
    print("reader families (cells, exact, deferred):", sizes)
    print("exact", exact, "deferred", deferred, "per e10 min", min(exact_e10[e] for e in range(-22, 23)))
    assert exact >= 15000 and deferred >= 8000
    assert sorted(exact_e10) == list(range(-22, 23)) and all(exact_e10[e] >= 100 for e in range(-22, 23)), sorted(exact_e10.items())
    # R3: the exact product needs 54 bits and its last one is set -- halfway between two doubles -- for every j
    pairs = F.r3_pairs()
    assert len(pairs) >= 800 and {j for _, j in pairs} == set(range(1, 23))
    for (m, j), text in zip(pairs, reader_texts("R3")):
        assert m % 2 == 1 and m <= 1 << 53 and 1 << 53 <= m * 5 ** j < 1 << 54 and text == b"%de%d" % (m, j)
        bits, late = read_cell(text)
        low = (m * 5 ** j - 1) // 2 << j + 1               # the two neighbours, both doubles: the even one is the answer
        ties = [float(low), float(low + (2 << j))]
        assert not late and F.from_bits(bits) in ties and (bits & 1) == 0 and abs(F.to_bits(ties[0]) - F.to_bits(ties[1])) == 1
    # R2: 2^53 is the last mantissa of the exact path, +-22 its last exponents
    for e, late in ((22, False), (-22, False), (23, True), (-23, True)):
        text = b"%de%d" % (1 << 53, e)
        assert text in reader_texts("R2") and read_cell(text)[1] == late
    assert read_cell(b"%de0" % ((1 << 53) + 1))[1] and b"%de0" % ((1 << 53) + 1) in reader_texts("R2")
    # R5 is no float, and sits about one per 64 rows
    assert all(read_cell(t) is None for t in F.R5)
    mixed = reader_texts("all+R5")
    nulls = [r for r, t in enumerate(mixed) if read_cell(t) is None]
    assert nulls == list(range(0, len(mixed), 64)) and {mixed[r] for r in nulls} == set(F.R5)
    assert [t for t in mixed if read_cell(t) is not None] == list(reader_texts("all"))
    assert sorted(reader_texts("all", "shuffled")) == sorted(reader_texts("all")) and reader_texts("all", "shuffled") != reader_texts("all")


def test_the_integer_family():
    ints = F.integers()
    assert len(ints) == 4 * 19 + 2 and all(-(1 << 63) <= v < 1 << 63 for v in ints)
    for sign in (1, -1):
        lengths = Counter(len(str(abs(v))) for v in ints if v * sign > 0)
        assert sorted(lengths) == list(range(1, 20)) and all(lengths[n] >= 2 for n in range(1, 19)), lengths
    assert {10 ** 18, 10 ** 19 - 1} & set(ints) == {10 ** 18} and 10 ** 18 - 1 in ints     # 19 digits: 10^18 and INT64_MAX
    assert [W.cell_text(W.INT64, v, 0x2C, 0x22)[0] for v in ints] == [b"%d" % v for v in ints]
    assert [C.parse_int(b"%d" % v) for v in ints] == ints


# ---------------------------------------------------------------- the host build of the headers
def run_cases(exe, mode: str, stdin: bytes) -> list:
    r = subprocess.run([exe, mode], input=stdin, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.split(b"\n")[:-1]


def reader_lines(texts) -> list:
    out = []
    for t in texts:
        cell = read_cell(t)
        out.append(b"N" if cell is None else b"%s %016x" % (b"D" if cell[1] else b"X", cell[0]))
    return out


def writer_lines(bit_patterns) -> list:
    return [b"%s %s" % (b"D" if late else b"X", text) for text, late in map(write_cell, bit_patterns)]


def differences(got, want, cells):
    assert len(got) == len(want), (len(got), len(want))
    return [(c, g, w) for c, g, w in zip(cells, got, want) if g != w]


def test_the_host_compiled_headers_give_the_restatements_answers(built_lib, tmp_path):
    """Every cell of every family through parse_float / exact_value and through float_form / form_text as g++ compiles
    them: the bits, the text and the deferred flag are the restatement's (a deferred cell's answer is the host's own
    conversion, which a call gives too). Then the same program under -fsanitize=address,undefined over the small
    families (a program of its own; nothing is loaded into python under a sanitizer)."""
    from oxen_amd import build

    build.build_host()
    texts = list(reader_texts("all+R5"))
    assert not any(b"\n" in t for t in texts)
    bad = differences(run_cases(build.CSV_FLOAT_CASES, "read", b"\n".join(texts) + b"\n"), reader_lines(texts), texts)
    assert not bad, (len(bad), bad[:5])
    patterns = SPECIAL_BITS + [F.to_bits(v) for name in ("W1", "W2", "W3", "W4") for v in writer_values(name)]
    got = run_cases(build.CSV_FLOAT_CASES, "write", struct.pack("<%dQ" % len(patterns), *patterns))
    bad = differences(got, writer_lines(patterns), patterns)
    assert not bad, (len(bad), bad[:5])
    print("host build: %d texts and %d doubles, no difference" % (len(texts), len(patterns)))
    exe = str(tmp_path / "csv_float_cases_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, build.CSV_FLOAT_CASES_SRC], check=True, timeout=300)
    texts = [t for name in ("R2", "R3", "R4", "R5") for t in reader_texts(name)]
    assert run_cases(exe, "read", b"\n".join(texts) + b"\n") == reader_lines(texts)
    patterns = SPECIAL_BITS + [F.to_bits(v) for name in ("W2", "W3") for v in writer_values(name)]
    assert run_cases(exe, "write", struct.pack("<%dQ" % len(patterns), *patterns)) == writer_lines(patterns)
