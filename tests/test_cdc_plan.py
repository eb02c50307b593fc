"""The FastCDC section planner on the CPU (oxen_amd/csrc/fastcdc_plan.hpp) through its native test
program, tests/native/cdc_plan_test.cpp: the scan / walk choice, section size, warm-up, capacities and
section table of planned calls, the walk's 4 GiB window and LDS rules, the error texts, and the
planner's invariants over a lattice of sizes and levels. Needs no GPU."""
import subprocess


def test_planner_native_program(built_lib):
    from oxen_amd import build

    build.build_host()
    r = subprocess.run([build.PLAN_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "checks passed" in r.stdout
