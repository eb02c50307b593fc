"""SNAPPY Parquet files on the GPU (oxh_parquet_* with OXH_PARQUET_INFLATE): pyarrow's fixtures
(tests/golden/make_df_parquet_snappy.py: V1 pages compressed whole, V2 pages with stored levels, dictionaries, pages
that grow) read bit for bit as the cells of tests/_parquet_cases.py in both forms; without the flag they are refused."""
import numpy as np
import pytest
import torch

import _parquet_cases as K
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
FILES = ("snappy_v1_dict_fallback", "snappy_v2_dict_fallback", "snappy_v2_plain")


@pytest.fixture(scope="module")
def want():   # the fixtures' cells, computed once and left alone
    return K.wanted(K.COLUMNS, K.cells(K.ROWS))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", FILES)
def test_snappy_fixtures_read_as_their_cells(ctx, want, name, form):
    data = K.fixture_bytes(name)
    if form == "host":
        got = tabular.read_parquet(data, ctx=ctx)
    else:   # the caller's bytes at an odd address
        d_data = torch.from_numpy(np.frombuffer(b"\0" * 3 + data, dtype=np.uint8).copy()).to("cuda:0")[3:]
        got = tabular.read_parquet_device(d_data, ctx=ctx, stream=ctx.stream)
    assert list(got) == [c for c, _, _ in K.COLUMNS]
    for col in got:
        K.assert_same(got[col], want[col], (name, col))
    with tabular.ParquetFile(data, ctx=ctx) as f:
        pages = f.stats.data_pages + f.stats.dict_pages   # pyarrow stores a V2 page that would grow (is_compressed false); V1 has no such flag
        assert f.stats.rows == K.ROWS and (f.stats.pages_inflated == pages if "v1" in name else 0 < f.stats.pages_inflated < pages)
    with tabular.ParquetFile(K.fixture_bytes(name[len("snappy_"):]), ctx=ctx) as f:
        assert f.stats.pages_inflated == 0
    with pytest.raises(_capi.OxenError, match="compression codec 1"):
        tabular.read_parquet(data, ctx=ctx, inflate=False)
