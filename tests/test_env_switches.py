"""The library's OXH_* environment switches have one home and one document. Text only: no GPU, no
library load.

  * oxen_amd/csrc/env.hpp is the only file of oxen_amd/csrc that calls getenv;
  * the switches it (and the separate host library, oxen_amd/host) reads are exactly the rows of
    INTEGRATION.md's tables plus OXH_DEVICE, which INTEGRATION.md documents in prose;
  * the tests set no OXH_* variable that nothing reads.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oxen_amd", "csrc")
HOST = os.path.join(ROOT, "oxen_amd", "host")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources(d):
    return sorted(p for p in glob.glob(os.path.join(d, "*")) if p.endswith((".hip", ".cpp", ".hpp", ".h")))


def _switches_read():
    """OXH_* names that reach getenv: env.hpp's accessors pass them to its helpers (text / integer / real /
    flag), the host library calls getenv itself."""
    env = _read(os.path.join(CSRC, "env.hpp"))
    names = set(re.findall(r'\b(?:text|integer|real|flag)\(\s*"(OXH_[A-Z0-9_]+)"', env))
    for p in _sources(HOST):
        names |= set(re.findall(r'getenv\(\s*"(OXH_[A-Z0-9_]+)"', _read(p)))
    return names


def test_getenv_only_in_env_hpp():
    callers = [os.path.basename(p) for p in _sources(CSRC) if re.search(r"\bgetenv\s*\(", _read(p))]
    assert callers == ["env.hpp"]
    # and env.hpp's own calls are its helpers': every name goes through one of them
    env = _read(os.path.join(CSRC, "env.hpp"))
    assert not re.search(r'getenv\(\s*"', env), "a getenv of a literal name beside the helpers"
    assert len(re.findall(r"\bgetenv\s*\(", env)) == 4


def test_switches_are_the_documented_set():
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    rows = re.findall(r"^\| `(OXH_[A-Z0-9_]+)` \|", doc, flags=re.M)
    assert len(rows) == len(set(rows)), sorted(r for r in rows if rows.count(r) > 1)
    assert "$OXH_DEVICE" in doc
    read = _switches_read()
    assert "OXH_DEVICE" in read and "OXH_TRACE" in read
    documented = set(rows) | {"OXH_DEVICE"}
    assert read - documented == set(), "switches without a row in INTEGRATION.md"
    assert documented - read == set(), "rows in INTEGRATION.md that nothing reads"


def test_tests_set_only_live_switches():
    live = _switches_read()
    used = set()
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.basename(p) == os.path.basename(__file__):
            continue
        src = _read(p)
        used |= set(re.findall(r'setenv\(\s*"(OXH_[A-Z0-9_]+)"', src))
        used |= set(re.findall(r'environ\[\s*"(OXH_[A-Z0-9_]+)"\s*\]\s*=', src))
        # env= dicts: "OXH_X": value, OXH_X=value in dict(...) calls
        used |= set(re.findall(r'"(OXH_[A-Z0-9_]+)"\s*:', src))
        used |= set(re.findall(r"\b(OXH_[A-Z0-9_]+)\s*=(?!=)", src))
    used = {u for u in used if not _is_abi_constant(u)}
    doubles = {u for u in used if u.startswith("OXH_FAKE_")}  # read by tests/native/fake_*.cpp
    fakes = "".join(_read(p) for p in glob.glob(os.path.join(ROOT, "tests", "native", "fake_*.cpp")))
    assert all(u in fakes for u in doubles), sorted(u for u in doubles if u not in fakes)
    assert not [u for u in used if u.startswith("OXH_TEST_")], "the suite has no opt-in names of its own"
    assert used - doubles - live == set(), "tests set switches that nothing reads"
    assert used & live, "the scan found none of the switches the tests are known to set"


def _is_abi_constant(name):
    """OXH_OK, OXH_ERR_*, OXH_MODE_* ...: ABI constants of include/oxen_hash.h, not environment variables."""
    return re.search(r"\b%s\b" % re.escape(name), _read(os.path.join(ROOT, "include", "oxen_hash.h"))) is not None
