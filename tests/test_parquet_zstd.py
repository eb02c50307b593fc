"""ZSTD Parquet files on the GPU (oxh_parquet_* with OXH_PARQUET_INFLATE_ZSTD): pyarrow's fixtures
(tests/golden/make_df_parquet_zstd.py: the SNAPPY fixtures' table and variants with ZSTD pages, and one file whose
columns are SNAPPY and ZSTD in turn) read bit for bit as the cells of tests/_parquet_cases.py in both forms; without
the ZSTD flag they are refused by the codec's number."""
import numpy as np
import pytest
import torch

import _parquet_cases as K
import test_parquet_read_cpu as P
from oxen_amd import _capi, tabular

pytestmark = pytest.mark.gpu
FILES = ("zstd_v1_dict_fallback", "zstd_v2_dict_fallback", "zstd_v2_plain", "zstd_snappy_mixed")


@pytest.fixture(scope="module")
def want():   # the fixtures' cells, computed once and left alone
    return K.wanted(K.COLUMNS, K.cells(K.ROWS))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", FILES)
def test_zstd_fixtures_read_as_their_cells(ctx, want, name, form):
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
        assert f.stats.rows == K.ROWS and (f.stats.pages_inflated == pages if "v2" not in name else 0 < f.stats.pages_inflated <= pages)
    with pytest.raises(_capi.OxenError, match="compression codec 6"):
        tabular.read_parquet(data, ctx=ctx, inflate=False)
    rc, msg, untouched = P.open_host(data, flags=_capi.OXH_PARQUET_INFLATE)   # the SNAPPY flag alone does not admit ZSTD
    assert rc == _capi.OXH_ERR_INVALID and "compression codec 6" in msg and untouched, msg
