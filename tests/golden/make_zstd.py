"""Writes tests/golden/zstd/*.zst and manifest.json with pyarrow's Zstandard codec (run once, by hand; the tests need no
pyarrow). The plains are tests/_zstd_cases.py's, compressed at levels 1, 3 and 19; what libzstd's one-shot call never
writes is made from a good frame by rewriting its header (a Window_Descriptor without a content size; the checksum flag
with the checksum appended) or is assembled by hand (RLE literals with no sequence). This file parses headers only --
frame, block, literals section, sequence count and modes -- and records the census per fixture; it asserts that the
set holds every form the kernel reads, that libzstd inflates every fixture to its plain and that it refuses every
malformed patch the manifest lists."""
import json
import os
import sys
import zlib

import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _zstd_cases as Z  # noqa: E402

MASK = (1 << 64) - 1
P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def xxh64(data: bytes) -> int:
    """XXH64 with seed 0: a frame's content checksum is its low 32 bits."""
    rotl = lambda x, r: (x << r | x >> (64 - r)) & MASK  # noqa: E731
    rnd = lambda acc, lane: rotl((acc + lane * P2) & MASK, 31) * P1 & MASK  # noqa: E731
    n, at = len(data), 0
    if n >= 32:
        v = [(P1 + P2) & MASK, P2, 0, -P1 & MASK]
        while at + 32 <= n:
            v = [rnd(v[k], int.from_bytes(data[at + 8 * k:at + 8 * k + 8], "little")) for k in range(4)]
            at += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & MASK
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & MASK
    else:
        h = P5
    h = (h + n) & MASK
    while at + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[at:at + 8], "little")), 27) * P1 + P4) & MASK
        at += 8
    if at + 4 <= n:
        h = (rotl(h ^ int.from_bytes(data[at:at + 4], "little") * P1 & MASK, 23) * P2 + P3) & MASK
        at += 4
    for byte in data[at:]:
        h = rotl(h ^ byte * P5 & MASK, 11) * P1 & MASK
    h = (h ^ h >> 33) * P2 & MASK
    h = (h ^ h >> 29) * P3 & MASK
    return h ^ h >> 32


def header_end(frame: bytes) -> int:
    fhd = frame[4]
    single = fhd >> 5 & 1
    return 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]


def census(frame: bytes) -> dict:
    """The forms a frame holds, from its headers alone."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    single = fhd >> 5 & 1
    found = {"content_size_bytes": ((1 if single else 0), 2, 4, 8)[fhd >> 6], "window_descriptor": not single, "checksum": bool(fhd & 4),
             "blocks": [], "literals": [], "weights": [], "sequence_counts": [], "ll": [], "of": [], "ml": []}
    at, last = header_end(frame), False
    while not last:
        head = int.from_bytes(frame[at:at + 3], "little")
        last, kind, size = head & 1, head >> 1 & 3, head >> 3
        at += 3
        found["blocks"].append(("raw", "rle", "compressed")[kind])
        if kind != 2:
            at += size if kind == 0 else 1
            continue
        blk = frame[at:at + size]
        at += size
        form, lit = blk[0] >> 2 & 3, blk[0] & 3
        if lit < 2:
            found["literals"].append(("raw", "rle")[lit])
            bytes_ = (1, 2, 1, 3)[form]
            regen = int.from_bytes(blk[:bytes_], "little") >> (3 if bytes_ == 1 else 4)
            pos = bytes_ + (regen if lit == 0 else 1)
        else:
            bytes_, width = (3, 3, 4, 5)[form], (10, 10, 14, 18)[form]
            comp = int.from_bytes(blk[:bytes_], "little") >> (4 + width) & ((1 << width) - 1)
            found["literals"].append(("huffman", "treeless")[lit - 2] + ("_1" if form == 0 else "_4"))
            if lit == 2:
                found["weights"].append("direct" if blk[bytes_] >= 128 else "fse")
            pos = bytes_ + comp
        b0 = blk[pos]
        nseq = b0 if b0 < 128 else (b0 - 128 << 8) + blk[pos + 1] if b0 < 255 else blk[pos + 1] + (blk[pos + 2] << 8) + 0x7F00
        pos += 1 if b0 < 128 else 2 if b0 < 255 else 3
        found["sequence_counts"].append("0" if nseq == 0 else "below_128" if nseq < 128 else "128_and_more")
        if nseq:
            for k, code in enumerate(("ll", "of", "ml")):
                found[code].append(("predefined", "rle", "fse", "repeat")[blk[pos] >> (6 - 2 * k) & 3])
    return {k: sorted(set(v)) if isinstance(v, list) else v for k, v in found.items()} | {"nblocks": len(found["blocks"])}


WANTED = {"blocks": {"raw", "rle", "compressed"}, "literals": {"raw", "rle", "huffman_1", "huffman_4", "treeless_1", "treeless_4"},
          "weights": {"fse", "direct"}, "sequence_counts": {"0", "below_128", "128_and_more"},
          **{code: {"predefined", "rle", "fse", "repeat"} for code in ("ll", "of", "ml")}}

LEVELS = {"words_150000": (1, 3), "words_400000": (19,)}   # the others at 1, 3 and 19; these two for the set's size limit

# (fixture, offset, new byte, cause): one byte of a good frame changed. words_900_l3 is a 10-byte frame header (2-byte
# content size at 5), one Compressed block whose header is at 7, its literals header at 10, the Huffman tree
# description at 13, the sequence count at 328, the modes at 329, the offset table's description from 330 and the
# bitstream behind it. The last three are not chosen by meaning: they are bytes whose change makes the sequences decode
# to an offset beyond the output, to lengths past the frame's size, and to fewer bytes than it.
PATCHES = [("words_900_l3", 0, 0x29, "frame"),       # the magic
           ("words_900_l3", 5, 0x85, "header"),      # the content size
           ("words_900_l3", 8, 0xFF, "input"),       # the block's size: it leaves the frame
           ("words_900_l3", 7, 0xFF, "block"),       # the reserved block type
           ("words_900_l3", 13, 0x00, "literals"),   # a tree description of no bytes
           ("words_900_l3", 329, 0x2C, "table"),     # match lengths in Repeat mode with no table before
           ("words_900_l3", 328, 0x00, "sequences"), # a count of 0 with a section behind it
           ("words_900_l3", 328, 0x80, "offset"), ("words_900_l3", 330, 0x01, "overrun"), ("words_900_l3", 336, 0x40, "truncated")]


def main():
    out = Z.GOLDEN
    os.makedirs(out, exist_ok=True)
    plains = Z.plains()
    frames = {}   # name -> (plain name, frame, how)
    for name, plain in plains.items():
        seen = set()
        for level in LEVELS.get(name, (1, 3, 19)):
            data = pa.Codec("zstd", compression_level=level).compress(plain).to_pybytes()
            if data not in seen:   # small inputs give the same frame at every level
                frames["%s_l%d" % (name, level)] = (name, data, "pyarrow level %d" % level)
                seen.add(data)
    good = frames["words_900_l3"][1]
    assert good[4] >> 5 & 1, "a single-segment header"
    frames["words_900_window"] = ("words_900", good[:4] + bytes([0x00, 10 << 3]) + good[header_end(good):], "header rewritten: no content size, Window_Descriptor")
    checksum = (xxh64(plains["words_900"]) & 0xFFFFFFFF).to_bytes(4, "little")
    frames["words_900_checksum"] = ("words_900", good[:4] + bytes([good[4] | 4]) + good[5:] + checksum, "header rewritten: checksum flag, checksum appended")
    plains["five_a"] = b"AAAAA"
    frames["rle_literals_no_sequence"] = ("five_a", bytes.fromhex("28b52ffd20051d0000294100"), "assembled by hand: RLE literals, sequence count 0")
    codec, listing, total = pa.Codec("zstd"), {}, 0
    for name, (plain_name, data, how) in frames.items():
        plain = plains[plain_name]
        assert codec.decompress(data, decompressed_size=len(plain)).to_pybytes() == plain, name
        assert len(data) < 150_000, (name, len(data))
        total += len(data)
        listing[name] = {"plain": plain_name, "length": len(plain), "crc32": zlib.crc32(plain), "how": how, "census": census(data)}
        with open(os.path.join(out, name + ".zst"), "wb") as f:
            f.write(data)
    assert total < 600_000, total
    for key, wanted in WANTED.items():
        have = set().union(*(entry["census"][key] for entry in listing.values()))
        assert wanted <= have, (key, wanted - have)
    assert {1, 2, 4} <= {entry["census"]["content_size_bytes"] for entry in listing.values()}
    assert any(e["census"]["window_descriptor"] and e["census"]["content_size_bytes"] == 0 for e in listing.values())
    assert any(e["census"]["checksum"] for e in listing.values()) and any(e["census"]["nblocks"] > 1 for e in listing.values())
    for name, at, byte, cause in PATCHES:
        data = bytearray(frames[name][1])
        assert data[at] != byte
        data[at] = byte
        try:
            codec.decompress(bytes(data), decompressed_size=listing[name]["length"])
        except Exception:
            continue
        raise AssertionError("libzstd accepts the patch %r" % ((name, at, byte, cause),))
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump({"fixtures": listing, "patches": [list(p) for p in PATCHES]}, f, indent=1, sort_keys=True)
    print(len(listing), "fixtures,", total, "bytes")


if __name__ == "__main__":
    main()
