"""The JSON writer (oxh_write_json_*) must not depend on what its working memory held before: both forms and both
formats under oxh_set_scratch_poison 0x00 / 0xFF / 0x5A, as tests/test_scratch_contents.py does for the other
entries. The frame has deferred floats (the list and the slots are a block of the call's own) and a long escaped cell
(the whole wave's path); the complete output and stats4 are compared exactly with the restatement, whose text is
computed once for the three bytes, and oxh_scratch_poisoned_bytes() must have grown around the calls."""
import contextlib
import functools
import os

import pytest

from oxen_amd import _capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_jsonwrite_call", os.path.join(HERE, "_jsonwrite_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
J = K.J


@pytest.fixture(params=[0x00, 0xFF, 0x5A], ids=["0x00", "0xFF", "0x5A"])
def poison(request, ctx):
    L = _capi.lib()
    prev = L.oxh_set_scratch_poison(request.param)
    try:
        assert prev == -1, prev
        yield request.param
    finally:
        L.oxh_set_scratch_poison(-1)


@contextlib.contextmanager
def poisoned(what):
    """The calls inside must have filled some working memory: a case whose counter stands still is not wired."""
    L = _capi.lib()
    before = L.oxh_scratch_poisoned_bytes()
    yield
    assert L.oxh_scratch_poisoned_bytes() > before, (what, "no working allocation was poisoned")


@functools.lru_cache(maxsize=None)
def case():
    n = 2048 + 64 + 3   # more than one tile of the scan, and a last wave that is not full
    floats = [0.5, 0.1 + 0.2, 1e15, None, float("nan"), 5e-324, 12.25, -0.0]
    strings = [b"plain", b"two\nlines", None, b'say "hi"', b"", b"\x01\x02"]
    cells = [[r * 7 - 1000 if r % 13 else None for r in range(n)], [floats[r % len(floats)] for r in range(n)], [r % 3 == 0 for r in range(n)],
             [strings[r % len(strings)] for r in range(n)]]
    cells[3][5] = b"\n".join(b"line %d of a long cell" % k for k in range(60)) + b'"'
    names, types = [b"i", b"f", b"b", b's"'], [J.INT64, J.FLOAT64, J.BOOL, J.STRING]
    cols = [K.host_column(t, c) for t, c in zip(types, cells)]
    want = {fmt: J.write(names, types, cells, fmt) for fmt in K.FORMATS}
    assert want[J.LINES][1][2] > 100 and len(cells[3][5]) > 512
    return names, types, cols, want


@pytest.mark.parametrize("fmt", K.FORMATS, ids=["lines", "array"])
@pytest.mark.parametrize("form", K.FORMS)
def test_outputs_do_not_depend_on_what_the_scratch_held(ctx, poison, form, fmt):
    names, types, cols, want = case()
    with poisoned("json write"):
        got, stats = K.write(ctx, form, cols, types, names, fmt, misalign=poison % 16)
    assert stats == want[fmt][1], (hex(poison), stats, want[fmt][1])
    assert got == want[fmt][0], hex(poison)
