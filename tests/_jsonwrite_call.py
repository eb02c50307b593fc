"""What tests/test_json_write.py, tests/test_json_write_cpu.py and tests/test_json_write_scratch.py share: one raw call
of oxh_write_json_* into a buffer at a chosen misalignment that is as long as the measure said and has sentinel bytes
on both sides, and the list of refusals. The frames are tests/_csvwrite_call.py's `host_column` / `to_device` Columns;
the expected bytes come from tests/_jsonwrite.py, which this file does not help."""
import ctypes
import os

import numpy as np

from oxen_amd import _capi, tabular

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_csvwrite_call", os.path.join(HERE, "_csvwrite_call.py"))
C = _util.module_from_spec(_spec)
_spec.loader.exec_module(C)
J = C.load("_jsonwrite_restatement", os.path.join(HERE, "_jsonwrite.py"))
host_column, to_device, from_bits, to_bits = C.host_column, C.to_device, C.from_bits, C.to_bits
PAD, SENTINEL = C.PAD, C.SENTINEL
FORMS = ["host", "device"]
FORMATS = [J.LINES, J.ARRAY]


class Call:
    """The arguments of one oxh_write_json_* call, kept alive."""

    def __init__(self, form, cols, types, names, fmt=J.LINES, kinds=None):
        self.form, self.device = form, form == "device"
        self.cols = [to_device(c) for c in cols] if self.device else list(cols)
        self.keep = []
        self.nrows = cols[0].nrows if cols else 0
        self.ncols = len(cols)
        self.types = (ctypes.c_uint32 * max(self.ncols, 1))(*[int(t) for t in types])
        self.tables = list(tabular._tables(self.cols, self._ptr))
        if kinds is not None:
            self.tables[0] = (ctypes.c_uint32 * max(self.ncols, 1))(*kinds)
        raw = [bytes(n) for n in names]
        self.name_offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in raw], out=self.name_offsets[1:])
        self.name_bytes = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
        self.flags = fmt

    def _ptr(self, a):
        if a is None:
            return None
        if self.device:
            return a.data_ptr() if a.numel() else None
        a = np.ascontiguousarray(a)
        self.keep.append(a)
        return a.ctypes.data if a.size else None

    def run(self, ctx, out, capacity, size=None, stats=None, **change):
        """rc of one call; `change` replaces arguments by name (for the refusals)."""
        L = _capi.lib()
        size = ctypes.c_uint64(0) if size is None else size
        stats = (ctypes.c_uint64 * 4)() if stats is None else stats
        a = dict(ctx=None if ctx is None else ctx.handle, nrows=self.nrows, ncols=self.ncols, types=self.types, kinds=self.tables[0],
                 values=self.tables[1], offsets=self.tables[2], validity=self.tables[3], bits=self.tables[4],
                 names=self.name_bytes.ctypes.data, name_offsets=self.name_offsets.ctypes.data_as(_capi._u64p), flags=self.flags,
                 out=out, capacity=capacity, out_bytes=ctypes.byref(size), stats4=stats)
        a.update(change)
        args = list(a.values())
        if self.device:
            rc = L.oxh_write_json_device(*args, None if ctx is None else ctx.stream)
        else:
            rc = L.oxh_write_json_host(*args)
        self.size, self.stats = int(size.value), tuple(int(x) for x in stats)
        return rc


def write(ctx, form, cols, types, names, fmt=J.LINES, misalign=0):
    """(bytes, stats4): the measuring call, then the writing call into a buffer at `misalign` mod 16 that is exactly
    as long as the measure said, with sentinel bytes in front of it and PAD and more behind it, which must survive."""
    call = Call(form, cols, types, names, fmt)
    rc = call.run(ctx, None, 0)
    assert rc == _capi.OXH_OK, _capi.lib().oxh_last_error()
    need, measured = call.size, call.stats
    assert measured[0] == need
    if call.device:
        import torch

        big = torch.full((need + PAD + 48,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        at = 16 + (misalign - big.data_ptr()) % 16
        torch.cuda.synchronize()
        rc = call.run(ctx, big.data_ptr() + at, need)
        torch.cuda.synchronize()
        raw = big.cpu().numpy()
    else:
        big = np.full(need + PAD + 48, SENTINEL, dtype=np.uint8)
        at = 16 + (misalign - big.ctypes.data) % 16
        rc = call.run(ctx, big.ctypes.data + at, need)
        raw = big
    assert rc == _capi.OXH_OK, _capi.lib().oxh_last_error()
    assert (call.size, call.stats) == (need, measured), "the measure and the write disagree"
    assert (raw[:at] == SENTINEL).all() and (raw[at + need:] == SENTINEL).all(), "bytes outside the output were written"
    return raw[at:at + need].tobytes(), call.stats


# ---------------------------------------------------------------- the refusals, for both test files
def refusal_frame():
    cells = [[1, None, 3], [1.5, 2.5, None], [True, None, False], [b"a", b"", None], [b"x", None, b'y"z']]
    types = [J.INT64, J.FLOAT64, J.BOOL, J.STRING, J.STRING64]
    return [host_column(t, c) for t, c in zip(types, cells)], types, [b"i", b"f", b"b", b"s", b"S"]


def refusals(call):
    """Every refusal of the header's list that needs no device, in its order: (changed arguments, the message)."""
    n = call.ncols
    bad_type = (ctypes.c_uint32 * n)(1, 2, 9, 4, 5)
    kinds = [int(k) for k in call.tables[0]]
    wrong = lambda at, kind: (ctypes.c_uint32 * n)(*[kind if c == at else k for c, k in enumerate(kinds)])  # noqa: E731
    decreasing = np.array([0, 1, 2, 1, 4, 5], dtype=np.uint64)
    no_values = (ctypes.c_void_p * n)(*[None if c == 0 else call.tables[1][c] for c in range(n)])
    no_offsets = (ctypes.c_void_p * n)(*[None if c == 3 else call.tables[2][c] for c in range(n)])
    return [
        (dict(types=None), b"is NULL"), (dict(kinds=None), b"is NULL"), (dict(values=None), b"is NULL"), (dict(offsets=None), b"is NULL"),
        (dict(validity=None), b"is NULL"), (dict(bits=None), b"is NULL"), (dict(ncols=0), b"ncols is 0"),
        (dict(flags=2), b"unknown flags"), (dict(flags=3), b"unknown flags"), (dict(types=bad_type), b"unknown type 9"),
        (dict(kinds=wrong(0, _capi.OXH_COL_FIXED4)), b"column 0 of type 1 has kind 4"), (dict(kinds=wrong(1, _capi.OXH_COL_BOOL)), b"column 1 of type 2"),
        (dict(kinds=wrong(2, _capi.OXH_COL_FIXED1)), b"column 2 of type 3"), (dict(kinds=wrong(3, _capi.OXH_COL_BYTES64)), b"column 3 of type 4"),
        (dict(kinds=wrong(4, _capi.OXH_COL_BYTES32)), b"column 4 of type 5"),
        (dict(name_offsets=None), b"name_offsets is NULL"), (dict(name_offsets=decreasing.ctypes.data_as(_capi._u64p)), b"name_offsets decrease"),
        (dict(names=None), b"names is NULL"), (dict(out_bytes=None), b"out_bytes or stats4"), (dict(stats4=None), b"out_bytes or stats4"),
        (dict(nrows=(1 << 40) + 1), b"2^40"), (dict(values=no_values), b"column 0 has no values"),
        (dict(offsets=no_offsets), b"column 3 is a byte column without offsets"),
    ], decreasing


def check_refusals(form, ctx, fmt=J.LINES):
    """Every refusal alone, then together with every later one: the call names the first. The outputs stay."""
    cols, types, names = refusal_frame()
    call = Call(form, cols, types, names, fmt)
    faults, keep = refusals(call)
    err = lambda: _capi.lib().oxh_last_error()  # noqa: E731
    out = np.full(256, SENTINEL, dtype=np.uint8)
    if call.device:
        import torch

        d_out = torch.full((256,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
    where = d_out.data_ptr() if call.device else out.ctypes.data
    for k, (change, what) in enumerate(faults):
        size, stats = ctypes.c_uint64(77), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        change = dict(change)
        if "out_bytes" not in change:
            change["out_bytes"] = ctypes.byref(size)
        rc = call.run(ctx, where, 256, size=size, stats=None if "stats4" in change else stats, **change)
        assert rc == _capi.OXH_ERR_INVALID and what in err() and err().startswith(b"json write:"), (k, change.keys(), err())
        assert size.value == 77 and list(stats) == [7] * 4, "a refused call wrote an output"
        later = {}
        for more, _ in reversed(faults[k + 1:]):
            later.update(more)
        later.update(change)
        rc = call.run(ctx, where, 256, size=size, stats=stats, **later)
        assert rc == _capi.OXH_ERR_INVALID and what in err(), (k, what, err())
        assert size.value == 77 and list(stats) == [7] * 4, "a refused call wrote an output"
    got = d_out.cpu().numpy() if call.device else out
    assert (got == SENTINEL).all()
    return call, where
