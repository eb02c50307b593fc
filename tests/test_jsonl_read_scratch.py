"""The JSON Lines reader (oxh_jsonl_*) must not depend on what its working memory held before: both forms under
oxh_set_scratch_poison 0x00 / 0xFF / 0x5A, as tests/test_json_write_scratch.py does for the writer. The frame has
deferred floats (the list and the slots are a block of the call's own), a long escaped cell, a non-canonical row
and a window that grows the schema (the listed rows' keys are a block of the call's own); the complete outputs are
compared exactly with the restatement, which parses once for the three bytes, and oxh_scratch_poisoned_bytes() must
have grown around the calls."""
import contextlib
import functools
import os

import pytest

from oxen_amd import _capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
from importlib import util as _util  # noqa: E402

_spec = _util.spec_from_file_location("_jsonl_call", os.path.join(HERE, "_jsonl_call.py"))
K = _util.module_from_spec(_spec)
_spec.loader.exec_module(K)
J = K.J
BS = chr(92)


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
    floats = ["0.5", "0.30000000000000004", "1e15", "null", "5e-324", "12.25", "-0", "123456789012345678901234567890"]
    rows = ['{"i":%d,"f":%s,"s":"row %d"}' % (r * 7 - 1000, floats[r % len(floats)], r) for r in range(n)]
    rows[5] = '{"i":5,"f":1e400,"s":"' + (BS + "n").join("line %d of a long cell" % k for k in range(60)) + BS + '""}'
    rows[70] = '{"s":"reordered","i":70,"late":true}'       # a non-canonical row; its key grows the schema inside the window
    rows[90] = '{"i":90,"f":1.,"s":"unparsable"'
    rows[200] = '{"i":200,"after":"the window"}'
    data = ("\n".join(rows) + "\n").encode()
    p = J.parse(data, 100)
    assert p.names == [b"i", b"f", b"s", b"late"] and p.stats8[3:] == (1, 0, 2, 1, 0) and J.column(p, 1, J.FLOAT64).stats4[2] > 100
    assert len(rows[5]) > 1024
    return data, p


@pytest.mark.parametrize("form", K.FORMS)
def test_outputs_do_not_depend_on_what_the_scratch_held(ctx, poison, form):
    data, p = case()
    with poisoned("jsonl read"):
        got = K.read(ctx, form, data, misalign=poison % 16, infer_rows=100)
    K.check(got, p, hex(poison))
