"""The single-launch Cholesky's planner without a GPU: its plans are the ones recorded before the planner moved into a header of its
own, and the header, built stand-alone with the host compiler, plans and replays clean under ASan + UBSan."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as entry
from gp_algos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_are_the_recorded_ones():
    """tests/golden/chol_plan_info.json: (ntasks, model_us) of gp_chol_plan_info for every shape
    test_single_launch_cholesky_plan_is_a_valid_schedule visits, recorded at commit 12a443f.  The task count is exact; the makespan
    to 1e-12 relative -- the same arithmetic, possibly inlined differently, while a schedule that changes at all moves it by whole
    task costs (9 us and up)."""
    entry.build()
    lib = _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "chol_plan_info.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 110
    nt, us = C.c_int(), C.c_double()
    for r in recorded:
        shape = (r["n"], r["extra_rows"], r["workgroups"])
        assert lib.gp_chol_plan_info(*shape, C.byref(nt), C.byref(us)) == _lib.GP_OK, shape
        assert nt.value == r["ntasks"], shape
        assert abs(us.value - r["model_us"]) <= 1e-12 * r["model_us"], (shape, us.value, r["model_us"])


def test_planner_is_asan_ubsan_clean_standalone(tmp_path):
    """tests/chol_plan_main.cpp over chol_plan.h alone, host g++ -fsanitize=address,undefined, run directly: plan + replay of
    nb = 1..41, 64, 112 block rows x extra in {0, 128} on 256 workers, and on 3 workers at nb in {5, 17, 41}.  The sanitizer runtimes
    are linked into the executable, so it starts whatever the environment it inherits preloads; the environment is passed on as it is
    (without the model's what-if costs)."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no host g++")
    for rt in ("libasan.a", "libubsan.a"):
        path = subprocess.run([gxx, "-print-file-name=" + rt], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path) or not os.path.exists(path):
            pytest.skip("host compiler has no static %s" % rt)
    exe = str(tmp_path / "chol_plan_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "gp_algos_amd", "csrc"), os.path.join(ROOT, "tests", "chol_plan_main.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "GPCORE_MEGA_COSTS"}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "92 plans, 0 bad" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
