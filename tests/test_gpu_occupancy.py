"""The forward pass of a policy on the GPU (csrc/vi_occupancy.h) against the numpy
restatement tests/occupancy_ref.py by array equality: mu, occ, ret and every row of mu_t, in both dtypes.

Shapes: 12 cells with no wall border (out-of-array neighbours, W != H), 63 (DistShift1, 9 x 7: one partial
wave), 81 (a second, partial wave), 361 (FourRooms: six waves, idle threads, the exchange crosses waves) and
1024 (no idle thread).  N = 40 covers full prefetch rounds; N = 7 and 8 an odd remainder and none.
"""
import functools

import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from minigrid_dynamicprogramming_amd.core import OBJECT_TO_IDX
from oracle import oracle
from tests import rollout_ref as rr
from tests import slip_ref as sr
from tests.occupancy_ref import OccupancyRef
from tests.test_occupancy_cpu import TOL32, TOL64, check_rollout_tie, stat_z

pytestmark = pytest.mark.gpu

E, WALL, GOAL, LAVA = (OBJECT_TO_IDX[k] for k in ("empty", "wall", "goal", "lava"))
ND = {"lava": "nodeath", "death_cost": -0.25}


@functools.lru_cache(maxsize=None)
def envs(env_id, B):
    enc, agent, env = rr.grids(env_id, B)
    return enc, agent, env, rr.cells_of(enc)


def random_policy(rows, B, S, seed):
    shape = (B, S) if rows == 1 else (rows, B, S)
    return np.random.default_rng(seed).integers(0, 7, shape).astype(np.int8)


def check(res, r):
    np.testing.assert_array_equal(res.mu, r["mu"])
    np.testing.assert_array_equal(res.occ, r["occ"])
    np.testing.assert_array_equal(res.ret, r["ret"])
    if r["mu_t"] is None:
        assert res.mu_t is None
    else:
        np.testing.assert_array_equal(res.mu_t, r["mu_t"])
    assert res.n_steps == r["n_steps"]
    for k in ("p_goal", "p_lava", "p_alive", "expected_return", "expected_steps"):
        np.testing.assert_array_equal(getattr(res, k), r[k], err_msg=k)
    for plane in (res.mu, res.occ, res.ret):
        assert not np.signbit(plane).any() or (plane[np.signbit(plane)] != 0).all()  # no -0


def both(cells, pol, start, kw, n_steps=None, every_step=False):
    """One pass on a fresh handle and in the restatement, compared; returns the GPU's result."""
    vi = mg.ValueIteration(cells, model="xyd", **kw)
    try:
        res = vi.occupancy(pol, start, n_steps=n_steps, every_step=every_step)
    finally:
        vi.close()
    check(res, OccupancyRef(cells, **kw).forward(pol, start, n_steps=n_steps, every_step=every_step))
    return res


# 6. a 3 x 4 grid whose rim holds goal and lava cells: their neighbours behind lie outside the array.  (The
# handle's loader refuses a walkable rim cell, so a live state never faces the edge itself on the GPU; the
# restatement's side of that case is tests/test_occupancy_cpu.py::test_cells_without_a_wall_border.)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("slip", [None, 0.9])
def test_rim_of_goal_and_lava_cells(dtype, slip):
    cells = np.array([[[WALL, GOAL, LAVA, WALL],
                       [LAVA, E, E, GOAL],
                       [WALL, WALL, GOAL, WALL]]], np.uint8)  # (H, W) = (3, 4): a transposed index lands elsewhere
    S = 48
    start = np.array([(1 * 4 + 1) * 4 + 1])  # cell (1, 1) facing down, into the wall: Fself is live
    fwd = np.full((1, S), 2, np.int8)
    res = both(cells, fwd, start, dict(dtype=dtype, slip_p=slip, gamma=0.95), n_steps=7, every_step=True)
    if slip is None:
        assert res.mu[0, start[0]] == 1.0  # it never leaves
    else:
        assert res.p_goal[0] > 0 and res.p_lava[0] > 0
    for seed, rows in ((1, 1), (2, 7)):
        both(cells, random_policy(rows, 1, S, seed), start, dict(dtype=dtype, slip_p=slip, horizon=7, gamma=1.0), every_step=True)
    mu0 = np.zeros((1, S))
    live = OccupancyRef(cells).live
    mu0[live] = 1.0 / live.sum()
    res = both(cells, np.minimum(random_policy(1, 1, S, 3), 2), mu0, dict(dtype=dtype, slip_p=slip, gamma=0.9), n_steps=8)
    assert res.p_goal[0] > 0 and res.p_lava[0] > 0  # every rim cell of the two kinds is entered from inside


# 7. grids on several waves, every option
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("env_id,B", [("MiniGrid-LavaCrossingS9N2-v0", 4), ("MiniGrid-FourRooms-v0", 2),
                                      ("MiniGrid-DistShift1-v0", 3)])
def test_every_option(env_id, B, dtype):
    enc, agent, _, cells = envs(env_id, B)
    start = rr.start_states(enc, agent, "xyd")
    H, S = 40, cells.shape[1] * cells.shape[2] * 4
    seed = 0
    for slip in (None, 0.9):
        for nd in ({}, ND):
            kw = dict(dtype=dtype, slip_p=slip, horizon=H, gamma=0.95, **nd)
            vi = mg.ValueIteration(cells, model="xyd", **kw)
            ref = OccupancyRef(cells, **kw)
            for rows in (1, H):
                seed += 1
                pol = random_policy(rows, B, S, seed)
                # (lanes 0..2 keep the mass moving: uniform lanes mostly stand still)
                pol = np.where(pol > 2, 2, pol).astype(np.int8) if seed % 2 else pol
                for every in (False, True):
                    check(vi.occupancy(pol, start, every_step=every), ref.forward(pol, start, every_step=every))
            vi.close()


# 8. exactly 1024 cells: no idle thread
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_1024_cells(dtype):
    cells = np.full((2, 32, 32), E, np.uint8)
    cells[:, 0, :] = cells[:, -1, :] = cells[:, :, 0] = cells[:, :, -1] = WALL
    cells[:, 30, 30] = GOAL
    cells[1, 5, 3:20] = LAVA
    S = 4096
    start = np.array([(1 * 32 + 1) * 4, (30 * 32 + 29) * 4])  # grid 1: one step from the goal
    for slip, rows in ((None, 8), (0.9, 1), (0.9, 8)):
        pol = np.minimum(random_policy(rows, 2, S, 11 + rows), 2).astype(np.int8)
        both(cells, pol, start, dict(dtype=dtype, slip_p=slip, gamma=0.9), n_steps=8, every_step=True)


# 9. a start distribution, and the duality against the GPU's own backward pass
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_uniform_start_distribution_and_the_gpus_own_evaluation(dtype):
    B, H = 2, 40
    enc, agent, _, cells = envs("MiniGrid-FourRooms-v0", B)
    kw = dict(dtype=dtype, slip_p=0.9, horizon=H, gamma=0.95)
    ref = OccupancyRef(cells, **kw)
    mu0 = np.zeros((B, ref.S), ref.T)
    for b in range(B):
        mu0[b, ref.live[b]] = ref.T(1) / ref.T(ref.live[b].sum())
    pi_t = oracle.value_iteration_ex(0, cells, gamma=0.95, slip_p=0.9, dtype=dtype, horizon=H, keep_policy_t=True)["pi_t"]
    vi = mg.ValueIteration(cells, model="xyd", **kw)
    res = vi.occupancy(pi_t, mu0)
    check(res, ref.forward(pi_t, mu0))
    vi.evaluate_opts(pi_t)
    v0 = vi.values().astype(np.float64)
    vi.close()
    dual = (mu0.astype(np.float64) * v0).sum(axis=1)
    print(dtype, "sum ret", res.expected_return, "<mu0, V0>", dual, "gap", np.abs(res.expected_return - dual).max())
    assert np.abs(res.expected_return - dual).max() <= (TOL32 if dtype == "f32" else TOL64)
    assert (res.expected_return > 0.05).all()


# 10. a plain handle: the discounted occupancy
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_plain_handle_discounted_occupancy(dtype):
    enc, agent, _, cells = envs("MiniGrid-LavaCrossingS9N2-v0", 3)
    start = rr.start_states(enc, agent, "xyd")
    pi = oracle.value_iteration(0, cells, gamma=0.9, slip_p=0.9, dtype="f64")["pi"]
    res = both(cells, pi, start, dict(dtype=dtype, slip_p=0.9, gamma=0.9), n_steps=50)
    # sum_t gamma^t * (live mass at t) <= (1 - gamma^50) / (1 - gamma)
    assert (res.expected_steps > 1.0).all() and (res.expected_steps < 10.0).all()
    both(cells, pi, start, dict(dtype=dtype, slip_p=0.9, gamma=0.9), n_steps=1, every_step=True)
    both(cells, np.stack([pi] * 3), start, dict(dtype=dtype, slip_p=0.9, gamma=0.9), n_steps=3)


# 11. the rollout tie on the GPU: without slip the pass is rollout()'s trajectory
@pytest.mark.parametrize("nodeath", [False, True])
def test_rollout_tie_against_the_gpu_rollout(nodeath):
    env_id, B = "MiniGrid-LavaCrossingS9N1-v0", 8
    enc, agent, env, cells = envs(env_id, B)
    H = env.max_steps
    kw = dict(gamma=1.0, dtype="f64", horizon=H, **(ND if nodeath else {}))
    pi_t = oracle.value_iteration_ex(0, cells, gamma=1.0, dtype="f64", lava_mode=int(nodeath), death_cost=-0.25,
                                     horizon=H, keep_policy_t=True)["pi_t"]
    pol = rr.noisy_policy(pi_t[0], "xyd", 0.5, lanes=3, T=H)  # env 1 walks into the lava
    venv = mg.MiniGridVecEnv(env_id, B, **({"no_death_types": ("lava",), "death_cost": -0.25} if nodeath else {}))
    venv.load(enc, agent)
    ro = venv.rollout(pol, trace=True)
    venv.close()
    assert ro.ok
    vi = mg.ValueIteration(cells, model="xyd", **kw)
    res = vi.occupancy(pol, rr.start_states(enc, agent, "xyd"), every_step=True)
    vi.close()
    check_rollout_tie({"mu_t": res.mu_t, "mu": res.mu}, {"steps": ro.steps, "states": ro.states}, B)
    np.testing.assert_array_equal(res.expected_return, ro.ret)
    np.testing.assert_array_equal(res.expected_steps, ro.steps.astype(float))
    assert (ro.ret[1] == 0.0 and ro.terminated[1]) if not nodeath else ro.ret[1] < ro.ret[0]


# 12. the Monte-Carlo tie on the GPU, against stat_case's cached reference outcomes
@pytest.mark.parametrize("env_id", ["MiniGrid-Empty-8x8-v0", "MiniGrid-LavaCrossingS9N1-v0"])
def test_monte_carlo_tie(env_id):
    c = sr.stat_case(env_id)
    cells = rr.cells_of(c["enc"][:1])
    start = rr.start_states(c["enc"][:1], c["agent"][:1], "xyd")
    res = both(cells, c["pi"][:1], start, dict(dtype="f64", slip_p=c["prob"], gamma=c["gamma"]), n_steps=c["max_steps"])
    z = stat_z(c, {"p_goal": res.p_goal, "p_lava": res.p_lava, "expected_return": res.expected_return})
    print(env_id, "z goal / lava / return", z)
    assert all(abs(x) <= 4.0 for x in z), z


# 13. errors, and the handle's state
def test_errors_leave_the_handle_usable_and_the_solve_untouched():
    B, H = 3, 6
    enc, agent, _, cells = envs("MiniGrid-LavaGapS5-v0", B)
    start = rr.start_states(enc, agent, "xyd")
    kw = dict(dtype="f32", horizon=H, gamma=0.95)
    ref = OccupancyRef(cells, **kw)
    vi = mg.ValueIteration(cells, model="xyd", **kw)
    good = random_policy(H, B, ref.S, 5)

    def usable():
        check(vi.occupancy(good, start, every_step=True), ref.forward(good, start, every_step=True))

    usable()  # before any solve
    pi = np.full((H, B, ref.S), 2, np.int8)
    v1, v2 = np.nonzero(ref.live[1])[0], np.nonzero(ref.live[2])[0]
    pi[4, 1, v1[3]] = 7
    pi[1, 1, v1[5]] = -1
    pi[1, 1, v1[9]] = 9
    pi[0, 2, v2[0]] = 7
    pi[:, 0, ~ref.live[0]] = 7
    with pytest.raises(ValueError, match=f"grid 1 t 1 state {v1[5]}: action -1 is outside \\[0, 7\\)"):
        vi.occupancy(pi, start)
    usable()
    pi[1, 1, v1[5]] = 2
    with pytest.raises(ValueError, match=f"grid 1 t 1 state {v1[9]}: action 9 "):
        vi.occupancy(pi, start, every_step=True)
    stat = np.full((B, ref.S), 2, np.int8)
    stat[2, v2[4]] = 7
    with pytest.raises(ValueError, match=f"grid 2 t 0 state {v2[4]}: action 7 "):
        vi.occupancy(stat, start)
    usable()
    flat = cells.reshape(B, -1)
    wall = int(np.nonzero(flat[1] == WALL)[0][0]) * 4
    goal = int(np.nonzero(flat[0] == GOAL)[0][0]) * 4 + 1
    lava = int(np.nonzero(flat[2] == LAVA)[0][0]) * 4 + 2
    for b, s in ((1, wall), (0, goal), (2, lava), (0, -1), (1, ref.S)):
        bad = start.copy()
        bad[b] = s
        with pytest.raises(ValueError, match=f"start: grid {b} state {s} "):
            vi.occupancy(good, bad)
    mu0 = np.zeros((B, ref.S), np.float32)
    mu0[np.arange(B), start] = 1
    mu0[1, goal], mu0[1, wall + 3] = 0.5, 0.25
    with pytest.raises(ValueError, match=f"mu0: grid 1 state {min(goal, wall + 3)} "):
        vi.occupancy(good, mu0)
    for T in (2, 5, 7):
        with pytest.raises(ValueError, match="T ="):
            vi.occupancy(np.full((T, B, ref.S), 2, np.int8), start)
    with pytest.raises(ValueError, match="n_steps"):
        vi.occupancy(good, start, n_steps=5)
    usable()
    # the pass touches no solve state: a solve after it is a fresh handle's
    k = vi.solve()
    V, P = vi.values(), vi.policy()
    fresh = mg.ValueIteration(cells, model="xyd", **kw)
    assert fresh.solve() == k
    np.testing.assert_array_equal(V, fresh.values())
    np.testing.assert_array_equal(P, fresh.policy())
    fresh.close()
    usable()  # ... and after one
    np.testing.assert_array_equal(vi.values(), V)
    np.testing.assert_array_equal(vi.policy(), P)
    vi.close()


def test_kernel_time_counts_the_launch():
    enc, agent, _, cells = envs("MiniGrid-LavaCrossingS9N2-v0", 4)
    vi = mg.ValueIteration(cells, model="xyd", dtype="f32", slip_p=0.9, horizon=40)
    pol = random_policy(40, 4, vi.S, 9)
    start = rr.start_states(enc, agent, "xyd")
    vi.enable_timing(True)
    ms0, n0 = vi.kernel_time()
    vi.occupancy(pol, start)
    ms1, n1 = vi.kernel_time()
    vi.occupancy(pol[0], start, every_step=True)
    ms2, n2 = vi.kernel_time()
    vi.close()
    assert (n1, n2) == (n0 + 1, n0 + 2) and ms2 > ms1 > ms0


def test_lone_served_grid_solves_the_same_around_a_pass():
    """A B = 1 plain handle may keep a resident server: the pass stops it, and the next solve is unchanged."""
    enc, agent, _, cells = envs("MiniGrid-LavaCrossingS9N1-v0", 1)
    vi = mg.ValueIteration(cells, model="xyd", dtype="f32")
    k = vi.solve()
    V, P = vi.values(), vi.policy()
    ref = OccupancyRef(cells, dtype="f32")
    start = rr.start_states(enc, agent, "xyd")
    check(vi.occupancy(P, start, n_steps=30), ref.forward(P, start, n_steps=30))
    np.testing.assert_array_equal(vi.values(), V)
    assert vi.solve() == k
    np.testing.assert_array_equal(vi.values(), V)
    np.testing.assert_array_equal(vi.policy(), P)
    vi.close()


def test_refusals():
    dk = envs("MiniGrid-DoorKey-5x5-v0", 1)
    vi = mg.ValueIteration(dk[0], model="doorkey", horizon=10)
    with pytest.raises(ValueError, match="rollout\\(trace=True\\)"):
        vi.occupancy(np.zeros((1, vi.S), np.int8), np.zeros(1, np.int64))
    vi.close()
    big = np.full((1, 33, 33), E, np.uint8)
    big[0, 0, :] = big[0, -1, :] = big[0, :, 0] = big[0, :, -1] = WALL
    big[0, 31, 31] = GOAL
    vi = mg.ValueIteration(big, model="xyd")
    with pytest.raises(ValueError, match="W\\*H <= 1024"):
        vi.occupancy(np.full((1, vi.S), 2, np.int8), np.array([(33 + 1) * 4]), n_steps=4)
    assert vi.solve() > 0
    vi.close()


def test_device_form_equals_the_host_form():
    import torch

    B, H = 4, 40
    enc, agent, _, cells = envs("MiniGrid-LavaCrossingS9N2-v0", B)
    start = rr.start_states(enc, agent, "xyd")
    kw = dict(dtype="f32", slip_p=0.9, horizon=H, gamma=0.95)
    vi = mg.ValueIteration(cells, model="xyd", **kw)
    pol = np.minimum(random_policy(H, B, vi.S, 3), 2).astype(np.int8)
    host = vi.occupancy(pol, start, every_step=True)
    dev = torch.device("cuda")
    d_pi = torch.from_numpy(pol).to(dev)
    d_start = torch.from_numpy(start.astype(np.int32)).to(dev)
    mu, occ, ret = (torch.empty((B, vi.S), dtype=torch.float32, device=dev) for _ in range(3))
    mu_t = torch.empty((H, B, vi.S), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert vi.occupancy_device(d_pi.data_ptr(), H, mu.data_ptr(), start_ptr=d_start.data_ptr(), occ_ptr=occ.data_ptr(),
                               ret_ptr=ret.data_ptr(), mu_t_ptr=mu_t.data_ptr()) == H
    for got, want in ((mu, host.mu), (occ, host.occ), (ret, host.ret), (mu_t, host.mu_t)):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    d_mu0 = torch.from_numpy(host.mu_t[0].copy()).to(dev)
    mu2 = torch.empty_like(mu)
    torch.cuda.synchronize()
    vi.occupancy_device(d_pi.data_ptr(), H, mu2.data_ptr(), mu0_ptr=d_mu0.data_ptr())  # occ, ret, mu_t NULL
    np.testing.assert_array_equal(mu2.cpu().numpy(), host.mu)
    with pytest.raises(ValueError, match="exactly one"):
        vi.occupancy_device(d_pi.data_ptr(), H, mu2.data_ptr())
    with pytest.raises(ValueError, match="aligned"):
        vi.occupancy_device(d_pi.data_ptr() + 4, H, mu2.data_ptr(), start_ptr=d_start.data_ptr())
    vi.close()
