"""What the Snappy tests share: a stream written from a list of elements, a plain byte-by-byte decoder of the raw
block format (include/oxen_hash.h "Snappy") as the reference, and one call of either form with the blocks at odd
addresses and guard bytes around the destinations."""
import ctypes

import numpy as np

PREAMBLE, INPUT, OFFSET_ZERO, OFFSET_BEYOND, OVERRUN, TRUNCATED = 1, 2, 3, 4, 5, 6
GUARD = 0xA5


class Malformed(Exception):
    pass


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 128:
        out.append(n & 127 | 128)
        n >>= 7
    return bytes(out + bytes([n]))


def emit(elements, declared=None) -> bytes:
    """The block of ("lit", bytes[, length bytes]) and ("copy", form 1 / 2 / 3, offset, length), in order."""
    out, total = bytearray(), 0
    for e in elements:
        if e[0] == "lit":
            n, wide = len(e[1]) - 1, e[2] if len(e) > 2 else 0
            if not wide and n < 60:
                out.append(n << 2)
            else:
                wide = wide or (n.bit_length() + 7) // 8
                out += bytes([(59 + wide) << 2]) + n.to_bytes(wide, "little")
            out += e[1]
            total += len(e[1])
        else:
            _, form, offset, length = e
            if form == 1:
                out += bytes([1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 255])
            else:
                out += bytes([form | (length - 1) << 2]) + offset.to_bytes(2 if form == 2 else 4, "little")
            total += length
    return varint(total if declared is None else declared) + bytes(out)


def inflate(block: bytes, want: int) -> bytes:
    """The reference: the block's bytes, or Malformed(cause)."""
    pos = declared = 0
    while True:
        if pos == len(block) or pos == 5:
            raise Malformed(PREAMBLE)
        declared |= (block[pos] & 127) << (7 * pos)
        pos += 1
        if not block[pos - 1] & 128:
            break
    if declared >= 1 << 32 or declared != want:
        raise Malformed(PREAMBLE)
    out = bytearray()
    while pos < len(block):
        tag = block[pos]
        form, high = tag & 3, tag >> 2
        extra = (high - 59 if high >= 60 else 0) if form == 0 else (1, 2, 4)[form - 1]
        if pos + 1 + extra > len(block):
            raise Malformed(INPUT)
        x = int.from_bytes(block[pos + 1:pos + 1 + extra], "little")
        pos += 1 + extra
        if form == 0:
            n = (x if extra else high) + 1
            if pos + n > len(block):
                raise Malformed(INPUT)
            if len(out) + n > declared:
                raise Malformed(OVERRUN)
            out += block[pos:pos + n]
            pos += n
            continue
        n, offset = (4 + (high & 7), (tag >> 5) << 8 | x) if form == 1 else (high + 1, x)
        if offset == 0:
            raise Malformed(OFFSET_ZERO)
        if offset > len(out):
            raise Malformed(OFFSET_BEYOND)
        if len(out) + n > declared:
            raise Malformed(OVERRUN)
        for _ in range(n):
            out.append(out[-offset])
    if len(out) != declared:
        raise Malformed(TRUNCATED)
    return bytes(out)


def run(ctx, blocks, wants, form):
    """(outputs, statuses, bad_blocks) of one call over the blocks, back to back from an odd address, into
    destinations back to back from an odd address inside a buffer of guard bytes, which must stay as they were."""
    from oxen_amd import _capi, tabular

    n, lead = len(blocks), 3
    src = np.frombuffer(b"\x55" * lead + b"".join(blocks), dtype=np.uint8).copy()
    src_offsets = (lead + np.concatenate([[0], np.cumsum([len(b) for b in blocks])])).astype(np.int64)
    dst_offsets = (5 + np.concatenate([[0], np.cumsum(wants)])).astype(np.int64)
    dst = np.full(int(dst_offsets[-1]) + 7, GUARD, dtype=np.uint8)
    status = np.full(n, 99, dtype=np.int32)
    if form == "host":
        bad = ctypes.c_uint64(99)
        u64 = lambda a: a.ctypes.data_as(_capi._u64p)  # noqa: E731
        _capi.check(_capi.lib().oxh_snappy_inflate_host(ctx.handle, n, src.ctypes.data, u64(src_offsets), dst.ctypes.data, u64(dst_offsets),
                                                        status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(bad)), "oxh_snappy_inflate_host")
        bad = bad.value
    else:
        import torch

        up = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
        d_dst, d_status = up(dst), up(status)
        bad = tabular.snappy_inflate_device(up(src), up(src_offsets), d_dst, up(dst_offsets), d_status, ctx=ctx, stream=ctx.stream)
        dst, status = d_dst.cpu().numpy(), d_status.cpu().numpy()
    assert np.all(dst[:5] == GUARD) and np.all(dst[int(dst_offsets[-1]):] == GUARD), "a guard byte was written"
    raw = dst.tobytes()
    return [raw[int(dst_offsets[k]):int(dst_offsets[k + 1])] for k in range(n)], [int(s) for s in status], bad
