"""oxh_add_files over items that share content: the blob is published once, and `stored` is 1 on the
FIRST item of each content whichever reader staged its copy first and whichever thread claimed it --
the same answer from the engine and from the caller-thread path (`stored` used to follow the race)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("direct", ["0", "1"], ids=["engine", "direct"])
def test_stored_marks_the_first_item_of_each_content(monkeypatch, ctx, oracle_lib, tmp_path, direct):
    from oxen_amd import hasher

    monkeypatch.setenv("OXH_DIRECT_FILES", direct)
    rng = np.random.default_rng(7)
    contents = [rng.integers(0, 256, 3000 + k, dtype=np.uint8).tobytes() for k in range(3)]
    n = 8 if direct == "1" else 96  # the caller-thread path takes at most 8 files
    which = [int(rng.integers(0, 3)) for _ in range(n)]
    paths = []
    for i, k in enumerate(which):
        paths.append(str(tmp_path / f"f{i}"))
        with open(paths[-1], "wb") as fh:
            fh.write(contents[k])
    for rep in range(3):
        root = str(tmp_path / f"versions{rep}")
        digests, sizes, st, stored = hasher.add_files(paths, root, ctx=ctx)
        assert list(st) == [0] * n
        assert [int(d) for d in digests] == [oracle_lib.xxh3_128_int(contents[k]) for k in which]
        assert [bool(s) for s in stored] == [which.index(k) == i for i, k in enumerate(which)]
        # the same call again finds every blob in place
        assert not any(hasher.add_files(paths, root, ctx=ctx)[3])
