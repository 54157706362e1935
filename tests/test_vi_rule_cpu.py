"""The global stopping rule that closes every solve and evaluation (csrc/vi_rule.h).

With exact arithmetic the contraction holds and the rule's loop never runs, so no GPU test reaches it; the
header is host-plain C++, so it is checked here: tools/vi_rule_check.cpp (its own main, nothing but
vi_rule.h) is built with the host compiler under AddressSanitizer + UBSan and driven with scripted dV
traces.  The fallback trace is tests/test_distributed_cpu.py's _NonMonotoneShard, which checks the same
rule as distributed.py restates it.
"""
import math
import os
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "minigrid_dynamicprogramming_amd", "csrc")
TOL = 1e-6
NON_MONOTONE = [1.0, 1e-3, 2e-6, 3e-6, 9e-7]  # dV(1..5): still >= tol at the locally chosen K = 3


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vi_rule") / "vi_rule_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tools", "vi_rule_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run_rule(exe, trace, K, max_sweeps=100, tol=TOL, horizon=0, fail_at=0, fail_code=0, reduce=False, null_out=False):
    row = [repr(tol), max_sweeps, horizon, K, fail_at, fail_code, int(reduce), int(null_out)] + [repr(float(x)) for x in trace]
    r = subprocess.run([exe], input=" ".join(str(x) for x in row) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    head, _, log = r.stdout.strip().partition(" :")
    rc, k, dv, converged, sweeps_out, dv_out, converged_out = head.split()
    return dict(rc=int(rc), k=int(k), dv=float(dv), converged=int(converged), outs=(int(sweeps_out), float(dv_out), int(converged_out)),
                calls=log.split())


def test_fallback_loop_finds_the_global_stopping_sweep(rule_exe):
    r = run_rule(rule_exe, NON_MONOTONE, K=3)
    assert r["calls"] == ["s4", "s5"]
    assert (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 5, 9e-7, 1)
    assert r["outs"] == (5, 9e-7, 1)


def test_fallback_loop_reduces_once_per_step_after_the_sweep(rule_exe):
    r = run_rule(rule_exe, NON_MONOTONE, K=3, reduce=True)
    assert r["calls"] == ["s4", "r4", "s5", "r5"]
    assert (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 5, 9e-7, 1)


def test_already_below_tol_takes_no_step(rule_exe):
    r = run_rule(rule_exe, NON_MONOTONE, K=5)
    assert r["calls"] == [] and (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 5, 9e-7, 1)


def test_dv_equal_to_tol_takes_a_step(rule_exe):
    r = run_rule(rule_exe, [1.0, TOL, 5e-7], K=2)  # the test is <, not <=
    assert r["calls"] == ["s3"] and (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 3, 5e-7, 1)


def test_cap_stops_unconverged_after_exactly_the_remaining_sweeps(rule_exe):
    r = run_rule(rule_exe, [1.0, 2e-6], K=3, max_sweeps=7)  # dV stays 2e-6 >= tol
    assert r["calls"] == ["s4", "s5", "s6", "s7"]
    assert (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 7, 2e-6, 0) and r["outs"] == (7, 2e-6, 0)


def test_nan_runs_to_the_cap_and_is_not_converged(rule_exe):
    r = run_rule(rule_exe, [1.0, float("nan")], K=2, max_sweeps=6)
    assert r["calls"] == ["s3", "s4", "s5", "s6"]
    assert (r["rc"], r["k"], r["converged"]) == (0, 6, 0) and math.isnan(r["dv"]) and math.isnan(r["outs"][1])


def test_error_stops_the_loop_at_once_with_k_at_the_last_completed_sweep(rule_exe):
    r = run_rule(rule_exe, [1.0, 1e-3, 2e-6, 3e-6, 4e-6, 9e-7], K=3, fail_at=5, fail_code=-3)
    assert r["calls"] == ["s4", "s5"]  # sweep 5 failed: no sweep 6
    assert (r["rc"], r["k"], r["dv"]) == (-3, 4, 3e-6)
    assert r["converged"] == -1 and r["outs"] == (-1, -1.0, -1)  # nothing was reported


def test_finite_horizon_reports_converged_whatever_dv_is(rule_exe):
    r = run_rule(rule_exe, [0.5], K=16, max_sweeps=16, horizon=16)
    assert r["calls"] == [] and (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 16, 0.5, 1) and r["outs"] == (16, 0.5, 1)
    r = run_rule(rule_exe, [float("nan")], K=16, max_sweeps=16, horizon=16)
    assert r["converged"] == 1 and r["outs"][2] == 1


def test_report_accepts_null_out_parameters(rule_exe):
    r = run_rule(rule_exe, NON_MONOTONE, K=3, null_out=True)
    assert (r["rc"], r["k"], r["dv"], r["converged"]) == (0, 5, 9e-7, 1)
    assert r["outs"] == (-1, -1.0, -1)  # the tool's own placeholders: the report wrote through no pointer
