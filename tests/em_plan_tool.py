"""Builds tests/native/em_plan_driver.cpp with the host compiler and runs it: the plan gbrs_amd/csrc/em_plan.h resolves for
one EM handle under a set of GBRS_TUNING_* variables.  Shared by tests/test_em_plan_cpu.py (the plan's own rows) and
tests/test_em_tiny_cpu.py (the limits the tiny cases were aimed at).  The same for tests/native/em_step_driver.cpp: the
route gbrs_amd/csrc/em_step.h resolves for one pass over such a handle (tests/test_em_step_route_cpu.py)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

with open(os.path.join(ROOT, "include", "gbrs_hip.h")) as _f:
    FLAG = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define GBRS_EM_(\w+) (\d+)u", _f.read())}
N_CU = 256


def build_driver(directory, name="em_plan_driver"):
    """Path of the driver compiled into `directory`; skips the calling test when there is no host C++ compiler."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def tuned_env(tuning):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GBRS_TUNING_")}
    env.update({"GBRS_TUNING_" + k: str(v) for k, v in tuning.items()})
    return env


def plan(driver, H=8, L=400, R=20000, N=100000, flags=(), counts=0, n_cu=N_CU, rule=None, **tuning):
    env = tuned_env(tuning)
    args = [driver, H, L, R, N, sum(FLAG[f] for f in flags), counts, n_cu] + ([rule] if rule else [])
    run = subprocess.run([str(a) for a in args], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0, run.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in run.stdout.split())}


def route(driver, kind="step", H=8, L=400, N=100000, flags=(), counts=0, n_tiles=5, n_long=0, all_one_word=0, acc_out=0,
          **tuning):
    """The route of one pass (em_step_driver): the enums by name, the rest as integers."""
    args = [driver, H, L, N, sum(FLAG[f] for f in flags), counts, kind, n_tiles, n_long, all_one_word, acc_out]
    run = subprocess.run([str(a) for a in args], capture_output=True, text=True, env=tuned_env(tuning), timeout=60)
    assert run.returncode == 0, run.stderr
    return {k: v if v.isalpha() or "_" in v else int(v) for k, v in (kv.split("=") for kv in run.stdout.split())}
