"""The Parquet reader (oxh_parquet_*) must not depend on what its working memory or its outputs held: each form
reads every fixture under oxh_set_scratch_poison and an output fill of 0x00, 0xFF and 0x5A (tests/test_parquet_write_scratch.py's
twin). The three results are identical and are the fixtures' cells."""
import ctypes

import numpy as np
import pytest
import torch

import _parquet_cases as K
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():   # the fixtures' cells, computed once and left alone
    return K.wanted(K.COLUMNS, K.cells(K.ROWS))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", K.FILES)
def test_outputs_do_not_depend_on_what_the_scratch_held(ctx, want, name, form):
    data = K.fixture_bytes(name)
    L, seen, device = _capi.lib(), set(), form == "device"
    source = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0") if device else data
    for poison in (0x00, 0xFF, 0x5A):
        assert L.oxh_set_scratch_poison(poison) == -1
        try:
            before = L.oxh_scratch_poisoned_bytes()
            with tabular.ParquetFile(source, ctx=ctx, device=device, stream=ctx.stream if device else None) as f:
                types = [t.type for t in f.types()]
                sizes, _ = f.measure(range(len(types)), types)
                # the outputs pre-filled: ParquetFile.columns with buffers of this test's making
                if device:
                    fill = lambda count, dtype: torch.full((count * np.dtype(dtype).itemsize,), poison, dtype=torch.uint8, device="cuda:0").view(getattr(torch, dtype))  # noqa: E731
                else:
                    fill = lambda count, dtype: np.full(count * np.dtype(dtype).itemsize, poison, dtype=np.uint8).view(dtype)  # noqa: E731
                cols = []
                for (_, dtype, _), size in zip(K.COLUMNS, sizes):
                    n, validity = K.ROWS, fill((K.ROWS + 7) // 8, "uint8")
                    if dtype == "str":
                        cols.append(tabular.Column(_capi.OXH_COL_BYTES32, n, fill(size, "uint8"), fill(n + 1, "int32"), validity))
                    elif dtype == "bool":
                        cols.append(tabular.Column(_capi.OXH_COL_BOOL, n, fill((n + 7) // 8, "uint8"), None, validity))
                    else:
                        cols.append(tabular.Column(int(dtype[2]), n, fill(n, {"<i8": "int64", "<i4": "int32", "<f4": "float32", "<f8": "float64"}[dtype]), None, validity))
                ptr = (lambda t: None if t is None else t.data_ptr()) if device else (lambda a: None if a is None else a.ctypes.data)
                m = len(cols)
                tables = [(ctypes.c_void_p * m)(*[ptr(getattr(c, field)) for c in cols]) for field in ("values", "offsets", "validity")]
                _, _, col_idx, type_words = f._selection(range(m), types)
                _, stats = f._call(m, col_idx, type_words, np.array(sizes, dtype=np.uint64), *tables)
            assert L.oxh_scratch_poisoned_bytes() > before, "no working allocation was poisoned"
        finally:
            L.oxh_set_scratch_poison(-1)
        for col, (cname, _, _) in zip(cols, K.COLUMNS):
            K.assert_same(col, want[cname], (name, cname, poison))
        seen.add((tuple(stats), tuple(K.to_host(c).values.tobytes() for c in cols)))
    assert len(seen) == 1, "the columns depend on what the scratch or the outputs held"

