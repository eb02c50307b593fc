"""The Parquet writer (oxh_write_parquet_*) must not depend on what its working memory or its output held: each form
writes one frame under oxh_set_scratch_poison and an output fill of 0x00, 0xFF and 0x5A (tests/test_json_write_scratch.py's
twin). The three files are identical and read back to the frame; the byte behind out_bytes keeps its fill."""
import numpy as np
import pytest
import torch

import _csvwrite_call as C
import test_parquet_write as T
from oxen_amd import _capi, tabular
from oxen_amd.device import _stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", ["host", "device"])
def test_outputs_do_not_depend_on_what_the_scratch_held(ctx, form):
    n = 3 * 1024 + 64 + 3   # four tiles, a last wave that is not full
    cells = [[r * 7 - 1000 if r % 13 else None for r in range(n)], [[0.5, None, float("nan"), -0.0][r % 4] for r in range(n)],
             [None if r % 5 == 2 else r % 3 == 0 for r in range(n)], [[b"plain", None, b"", b"\x01\x02"][r % 4] for r in range(n)]]
    cells[3][5] = b"a long cell " * 60
    types = [C.W.INT64, C.W.FLOAT64, C.W.BOOL, C.W.STRING]
    cols = [C.host_column(t, c, vbit=3, nbit=5) for t, c in zip(types, cells)]
    frame = dict(zip("ifbs", [C.to_device(c) for c in cols] if form == "device" else cols))
    head = tabular._parquet_head(frame, 2048, 12000, types)
    ptr = (lambda t: None if t is None else t.data_ptr()) if form == "device" else (lambda a: None if a is None else a.ctypes.data)
    L, seen = _capi.lib(), set()
    fixed = (getattr(L, "oxh_write_parquet_" + form), "parquet write", ctx, *head[:2], tabular._tables(head[0], ptr), *head[2:])
    stream = [_stream(ctx.stream)] if form == "device" else []
    for poison in (0x00, 0xFF, 0x5A):
        assert L.oxh_set_scratch_poison(poison) == -1
        try:
            before = L.oxh_scratch_poisoned_bytes()
            need, measured = tabular._write_call(*fixed, None, 0, *stream)
            out = torch.full((need + 1,), poison, dtype=torch.uint8, device="cuda:0") if form == "device" else np.full(need + 1, poison, dtype=np.uint8)
            again = tabular._write_call(*fixed, out.data_ptr() if form == "device" else out.ctypes.data, need, *stream)
            assert L.oxh_scratch_poisoned_bytes() > before, "no working allocation was poisoned"
        finally:
            L.oxh_set_scratch_poison(-1)
        got = out.cpu().numpy() if form == "device" else out
        assert again == (need, measured) and got[need] == poison, "the byte behind out_bytes was written"
        seen.add((got[:need].tobytes(), tuple(measured)))   # (data, stats4): check()'s first and last arguments
    assert len(seen) == 1, "the file depends on what the scratch or the output held"
    T.check(*seen.pop(), cols, types, [b"i", b"f", b"b", b"s"])
