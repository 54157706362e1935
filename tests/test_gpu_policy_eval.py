"""Policy evaluation, greedy improvement and policy iteration on the GPU (vi_eval_kernel,
vi_improve_kernel) against the numpy restatement tests/policy_ref.py: V and pi bit for bit
(assert_array_equal), sweeps, dV, converged and the per-grid executed sweeps.

Shapes are the smallest at which the kernel can still go wrong: 5x5 (under one wave), 8x8 (exactly one
wave), 9x9 (a partial second wave), 7x13 (not square), FourRooms 19x19, a random-obstacle 33x33 (1089
cells: more than one cell per thread, topology and lanes re-read from LDS), DoorKey 8x8 and 16x16, and a
hand-built DoorKey 33x33 in fp32 (the same strided path with 16 lanes per cell, 158 KB of LDS).
Batches: a lone grid with a server resident, 3, 65, and 513 grids of 5x5 (past the in-launch
reduction's limit: the reduce kernel's path).
"""
import functools

import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from oracle import oracle
from tests.policy_ref import PolicyRef
from tests.test_gpu_wave2 import random_grids

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
TOL, GAMMA = 1e-6, 0.99


@functools.lru_cache(maxsize=None)
def fourrooms():
    env = mg.make("MiniGrid-FourRooms-v0")
    return np.stack([env.generate(seed=s)[0][..., 0].T for s in range(4)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def doorkey(size, n):
    env = mg.make(f"MiniGrid-DoorKey-{size}x{size}-v0")
    return np.stack([env.generate(seed=s)[0][..., 0].T for s in range(n)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def big_doorkey(W=33, H=33, n=2):
    """DoorKey grids of more than 1024 cells: a wall column with the locked door, the key on its left,
    the goal in the last rows on its right (cells at flat index >= 1024 matter), random walls elsewhere."""
    rng = np.random.default_rng(5)
    out = np.full((n, H, W), 2, np.uint8)
    for i in range(n):
        g = out[i]
        g[1:-1, 1:-1] = rng.choice(np.array([1, 1, 1, 1, 1, 1, 2], np.uint8), size=(H - 2, W - 2))
        x, dy = W // 2 + i, 5 + 3 * i
        g[1:-1, x] = 2
        g[dy, x - 1:x + 2] = (1, 4, 1)
        g[H - 6, 3 + i] = 5
        g[H - 2 - i, W - 2] = 8
    return out


@functools.lru_cache(maxsize=None)
def xyd_grids(W, H, B):
    return random_grids(B, W, H, seed=W * 31 + H, goals=2)


@functools.lru_cache(maxsize=None)
def ref_of(key, model, dtype, slip, gamma=GAMMA):
    """One PolicyRef per (grids, dtype, slip, gamma), shared by the tests (they do not modify it)."""
    cells = {"fr": fourrooms, "dk8": lambda: doorkey(8, 4), "dk16": lambda: doorkey(16, 3), "dk33": big_doorkey}[key]() \
        if isinstance(key, str) else xyd_grids(*key)
    return cells, PolicyRef(model, cells, gamma=gamma, tol=TOL, slip_p=slip, dtype=dtype)


@functools.lru_cache(maxsize=None)
def pi_star(key, model, dtype):
    """pi* of the deterministic problem, from the oracle (the GPU solve's is compared with it elsewhere)."""
    cells, _ = ref_of(key, model, dtype, None)
    return oracle.value_iteration(model, cells, dtype=dtype, fixed_point=True)


def random_policy(ref, seed):
    return np.random.default_rng(seed).integers(0, ref.A, (ref.B, ref.S)).astype(np.int8)


def check(vi, r):
    assert vi.sweeps == r["sweeps"]
    assert vi.dv == r["dv"]
    assert vi.converged == r["converged"]
    np.testing.assert_array_equal(vi.values(), r["V"])
    np.testing.assert_array_equal(vi.policy(), r["pi"])
    np.testing.assert_array_equal(vi.grid_sweeps(), r["grid_sweeps"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W,H", [(5, 5), (8, 8), (9, 9), (7, 13), (33, 33)])
def test_xyd_shapes_random_and_uniform_policies(W, H, dtype):
    """B = 3, deterministic and slip 0.9 (at gamma 0.95): a seeded random policy, the uniform "forward"
    and the deterministic pi* (the policy with the longest deterministic evaluations)."""
    for slip, gamma in ((None, GAMMA), (0.9, 0.95)):
        cells, ref = ref_of((W, H, 3), 0, dtype, slip, gamma)
        vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip, gamma=gamma)
        try:
            for pi in (random_policy(ref, 7), np.full((ref.B, ref.S), 2, np.int8), pi_star((W, H, 3), 0, dtype)["pi"]):
                vi.evaluate(pi)
                check(vi, ref.evaluate(pi))
        finally:
            vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key,model", [("fr", 0), ("dk8", 1), ("dk16", 1)])
def test_pi_star_reproduces_the_solve(key, model, dtype):
    """Deterministic grids: evaluating the handle's own pi* (evaluate_device(None) right after solve())
    gives the solve's V, sweeps and grid_sweeps bit for bit; the grids' depths differ, so grid_sweeps
    differ while K is their maximum.  Then random and uniform policies on the same handle."""
    cells, ref = ref_of(key, model, dtype, None)
    o = pi_star(key, model, dtype)
    vi = mg.ValueIteration(cells, dtype=dtype)
    try:
        k = vi.solve()
        V, pi = vi.values(), vi.policy()
        np.testing.assert_array_equal(pi, o["pi"])
        assert vi.evaluate_device() == k
        r = ref.evaluate(pi)
        check(vi, r)
        np.testing.assert_array_equal(vi.values(), V)
        assert len(set(r["grid_sweeps"].tolist())) > 1 and r["grid_sweeps"].max() == k
        for p in (random_policy(ref, 3), np.full((ref.B, ref.S), 0, np.int8)):
            vi.evaluate(p)
            check(vi, ref.evaluate(p))
        # a solve after evaluations is the solve of a fresh handle: the oracle's, per-grid sweeps included
        assert vi.solve() == o["sweeps"] and vi.dv == o["dv"] and vi.converged
        np.testing.assert_array_equal(vi.values(), o["V"])
        np.testing.assert_array_equal(vi.policy(), o["pi"])
        np.testing.assert_array_equal(vi.grid_sweeps(), o["grid_sweeps"])
    finally:
        vi.close()


def test_doorkey_above_1024_cells():
    """DoorKey 33x33 fp32: 1089 cells strided over 1024 threads with 16 lanes per cell, 158 KB of LDS;
    (the largest DoorKey square a handle accepts: the evaluation's layout is the solve's, so every grid a
    fused handle holds can be evaluated); pi*, a random policy, improvement and policy iteration."""
    cells, ref = ref_of("dk33", 1, "f32", None)
    o = pi_star("dk33", 1, "f32")
    far = (o["V"].reshape(ref.B, -1, 16)[:, 1024:] > 0).any(axis=2).sum(axis=1)
    assert far.min() >= 8 and o["sweeps"] > 40, (far, o["sweeps"])  # the cells past one per thread matter
    vi = mg.ValueIteration(cells, dtype="f32", model="doorkey")
    try:
        for p in (o["pi"], random_policy(ref, 5)):
            vi.evaluate(p)
            r = ref.evaluate(p)
            check(vi, r)
        assert vi.improve() == ref.improve(r["V"], r["pi"])[1] > 0
        np.testing.assert_array_equal(vi.policy(), ref.improve(r["V"], r["pi"])[0])
        r = ref.policy_iteration(max_iters=3)
        out = vi.policy_iteration(max_iters=3)
        assert (out["iters"], out["eval_sweeps"], out["changed"]) == (3, r["eval_sweeps"], r["changed"])
        np.testing.assert_array_equal(vi.values(), r["V"])
        np.testing.assert_array_equal(vi.policy(), r["pi"])
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_lone_grid_with_a_resident_server(dtype):
    """B = 1: the second solve() leaves the persistent server resident; the evaluation stops it first.
    solve() afterwards equals a fresh handle's, and the protocol entry points need a reset."""
    cells = fourrooms()[:1]
    ref = PolicyRef(0, cells, dtype=dtype)
    vi = mg.ValueIteration(cells, dtype=dtype)
    try:
        assert vi.persistent
        vi.solve()
        k = vi.solve()
        V, pi = vi.values(), vi.policy()
        vi.solve()  # a server is resident again
        assert vi.evaluate_device() == k
        check(vi, ref.evaluate(pi))
        np.testing.assert_array_equal(vi.values(), V)
        p = random_policy(ref, 11)
        vi.solve()
        vi.evaluate(p)
        check(vi, ref.evaluate(p))
        with pytest.raises(ValueError, match="reset"):
            vi.run_to(k)
        with pytest.raises(ValueError, match="reset"):
            vi.sweep()
        assert vi.solve() == k
        np.testing.assert_array_equal(vi.values(), V)
        np.testing.assert_array_equal(vi.policy(), pi)
        vi.evaluate(p)
        vi.reset()
        assert vi.run_local() == k  # after a reset the protocol is the solve's again
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W,H,B", [(9, 9, 65), (5, 5, 513)])
def test_batches(W, H, B, dtype):
    """65 grids (the in-launch reduction) and 513 (one past its limit: the reduce kernel); the slip
    case at gamma 0.9 (about 130 sweeps: the reduction is the point)."""
    for slip, gamma in ((None, GAMMA), (0.9, 0.9)):
        cells, ref = ref_of((W, H, B), 0, dtype, slip, gamma)
        pi = random_policy(ref, B)
        vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip, gamma=gamma)
        try:
            vi.evaluate(pi)
            check(vi, ref.evaluate(pi))
        finally:
            vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slip", [0.9, 0.5])
def test_deterministic_pi_star_under_slip(slip, dtype):
    """What pi*_det is worth when actions slip: a real linear system, hundreds of sweeps."""
    cells, ref = ref_of("fr", 0, dtype, slip)
    pi = pi_star("fr", 0, dtype)["pi"]
    r = ref.evaluate(pi)
    assert r["sweeps"] > 50 and 0.0 < r["dv"] < TOL
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip)
    try:
        vi.evaluate(pi)
        check(vi, r)
        res = vi.result()
        assert res.sweeps == r["sweeps"] and res.converged
    finally:
        vi.close()
    m = mg.policy_evaluation(cells, pi, dtype=dtype, slip_p=slip)
    np.testing.assert_array_equal(m.V, r["V"])
    assert m.sweeps == r["sweeps"] and m.dv == r["dv"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_sweeps_cap(dtype):
    """A 600-sweep slip evaluation capped at 7: converged == 0 and V is the restatement's V_7."""
    cells, ref = ref_of("fr", 0, dtype, 0.5)
    pi = np.full((ref.B, ref.S), 2, np.int8)
    assert ref.evaluate(pi)["sweeps"] > 500
    r = ref.evaluate(pi, max_sweeps=7)
    assert r["sweeps"] == 7 and not r["converged"]
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=0.5, max_sweeps=7)
    try:
        vi.evaluate(pi)
        check(vi, r)
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_actions(dtype):
    """7 (XYD) / 5 (DoorKey) on a valid state: ValueError naming the first offending grid and state;
    the same value on absorbing states is accepted and stored as -1."""
    for key, model, badv in (("fr", 0, 7), ("dk8", 1, 5)):
        cells, ref = ref_of(key, model, dtype, None)
        vi = mg.ValueIteration(cells, dtype=dtype)
        try:
            pi = np.full((ref.B, ref.S), 2, np.int8)
            pi[ref.absorb] = badv
            vi.evaluate(pi)
            check(vi, ref.evaluate(pi))
            valid = np.argwhere(~ref.absorb)
            (b1, s1), (b2, s2) = valid[len(valid) // 2], valid[-1]  # grid b1 < b2: b1's is reported
            pi[b1, s1] = badv
            pi[b2, s2] = -3
            with pytest.raises(ValueError, match=f"grid {b1} state {s1}: action {badv}"):
                vi.evaluate(pi)
            pi[b1, s1] = 2
            with pytest.raises(ValueError, match=f"grid {b2} state {s2}: action -3"):
                vi.evaluate(pi)
            pi[b2, s2] = 1
            vi.evaluate(pi)  # the handle is usable after a refusal
            check(vi, ref.evaluate(pi))
        finally:
            vi.close()


def test_unsupported_handles_and_bad_arguments():
    cells = fourrooms()
    S = cells.shape[1] * cells.shape[2] * 4
    pi = np.full((4, S), 2, np.int8)
    for kw in ({"method": "sweep"}, {"horizon": 50}, {"lava": "nodeath"}):
        vi = mg.ValueIteration(cells, **kw)
        try:
            for call in (lambda: vi.evaluate(pi), vi.evaluate_device, vi.improve, vi.policy_iteration):
                with pytest.raises(ValueError):
                    call()
        finally:
            vi.close()
    vi = mg.ValueIteration(cells)
    try:
        with pytest.raises(ValueError, match="shape"):
            vi.evaluate(pi[:, :-4])
        with pytest.raises(ValueError, match="integer"):
            vi.evaluate(pi.astype(np.float32))
        with pytest.raises(ValueError, match="solve or evaluate"):
            vi.improve()
        with pytest.raises(ValueError):
            vi.policy_iteration(max_iters=0)
    finally:
        vi.close()


PI_CASES = [("fr", 0, None), ("fr", 0, 0.9), ("dk8", 1, None)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key,model,slip", PI_CASES)
def test_improve_step_by_step(key, model, slip, dtype):
    """evaluate() / improve() in a host loop: the changed count and pi of every iteration."""
    cells, ref = ref_of(key, model, dtype, slip)
    r = ref.policy_iteration()
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip)
    try:
        pi = np.full((ref.B, ref.S), 2, np.int8)
        for want in r["changes"]:
            vi.evaluate(pi)
            ev = ref.evaluate(pi)
            np.testing.assert_array_equal(vi.values(), ev["V"])
            assert vi.improve() == want
            pi = vi.policy()
            np.testing.assert_array_equal(pi, ref.improve(ev["V"], ev["pi"])[0])
        np.testing.assert_array_equal(pi, r["pi"])
        if slip is None:  # improvement on a solve's V (an exact fixed point): pi* is stable
            vi.solve()
            star = vi.policy()
            assert vi.improve() == 0
            np.testing.assert_array_equal(vi.policy(), star)
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key,model,slip", PI_CASES + [("fr", 0, 0.5)])
def test_policy_iteration(key, model, slip, dtype):
    cells, ref = ref_of(key, model, dtype, slip)
    r = ref.policy_iteration()
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip)
    try:
        out = vi.policy_iteration()
        assert out == {"iters": r["iters"], "eval_sweeps": r["eval_sweeps"], "changed": 0, "dv": r["dv"]}
        assert vi.sweeps == r["sweeps"] and vi.converged
        np.testing.assert_array_equal(vi.values(), r["V"])
        np.testing.assert_array_equal(vi.policy(), r["pi"])
        np.testing.assert_array_equal(vi.grid_sweeps(), r["grid_sweeps"])
        # against value iteration: both stop with dV < tol under a gamma-contraction, so each is within
        # tol*gamma/(1-gamma) of its fixed point, and the fixed points coincide
        V = vi.values()
        vi.solve()
        assert np.abs(V.astype(np.float64) - vi.values()).max() <= 2 * TOL * GAMMA / (1 - GAMMA)
        # from all-"done" (XYD) / all-"toggle" (DoorKey), and capped at one iteration
        start = np.full((ref.B, ref.S), ref.A - 1, np.int8)
        r1 = ref.policy_iteration(start, max_iters=1)
        out = vi.policy_iteration(start, max_iters=1)
        assert out["iters"] == 1 and out["changed"] == r1["changed"] > 0 and out["eval_sweeps"] == r1["eval_sweeps"]
        np.testing.assert_array_equal(vi.policy(), r1["pi"])
        np.testing.assert_array_equal(vi.values(), r1["V"])
    finally:
        vi.close()
    m = mg.policy_iteration(cells, dtype=dtype, slip_p=slip)
    assert (m.iters, m.eval_sweeps, m.changed, m.sweeps) == (r["iters"], r["eval_sweeps"], 0, r["sweeps"])
    np.testing.assert_array_equal(m.V, r["V"])
    np.testing.assert_array_equal(m.pi, r["pi"])
