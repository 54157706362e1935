"""Policy evaluation under NoDeath lava and finite horizons on the GPU, against
the numpy restatement tests/policy_opts_ref.py by array equality: V_0, V_t, the normalised pi, sweeps,
dv and grid_sweeps.

Shapes: 25 cells (one partly filled wave), 81 (a second, partial wave), 256 (four full waves), 1024
(the largest workgroup), DoorKey 5x5 and 8x8; B in {1, 3, 65}; H in {1, 2, 3, 7} (tile parity, no
prefetch, a prefetch shorter than its distance, one full round and a remainder) and the env's own
max_steps on the two smallest families.  The policies are uniform random lanes on every state, so every
action of every state kind is taken somewhere.
"""
import functools

import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from minigrid_dynamicprogramming_amd.dp import n_actions, state_index
from oracle import oracle
from tests import rollout_ref as rr
from tests.policy_opts_ref import PolicyOptsRef, lava_entries
from tests.policy_ref import PolicyRef

pytestmark = pytest.mark.gpu

MODEL_ID = {"xyd": 0, "doorkey": 1}


@functools.lru_cache(maxsize=None)
def envs(env_id, B):
    enc, agent, env = rr.grids(env_id, B)
    return enc, agent, env, rr.cells_of(enc)


@functools.lru_cache(maxsize=None)
def room32():
    """One 32 x 32 room, exactly 1024 cells: goal in a corner, a lava bar and a few inner walls; B = 3
    variants that differ in the bar's row."""
    out = []
    for b in range(3):
        c = np.full((32, 32), 1, np.uint8)   # empty
        c[0, :] = c[-1, :] = c[:, 0] = c[:, -1] = 2  # wall
        c[30, 30] = 8                         # goal
        c[10 + 3 * b, 3:25] = 9               # lava
        c[20, 5:31] = 2
        c[20, 17] = 1
        out.append(c)
    return np.stack(out)


def random_policy(rows, B, S, model, seed):
    rng = np.random.default_rng(seed)
    shape = (B, S) if rows == 1 else (rows, B, S)
    return rng.integers(0, n_actions(model), shape).astype(np.int8)


def handle(cells, model, **kw):
    return mg.ValueIteration(cells, model=model, **kw)


def ref_kw(kw):
    return {k: v for k, v in kw.items() if k in ("gamma", "tol", "slip_p", "dtype", "lava", "death_cost", "horizon")}


def check_horizon(vi, ref, pol, values_t):
    r = ref.evaluate_horizon(pol)
    k = vi.evaluate_opts(pol, values_t=values_t)
    assert k == vi.sweeps == r["sweeps"] and vi.converged and vi.dv == r["dv"]
    np.testing.assert_array_equal(vi.values(), r["V"])
    np.testing.assert_array_equal(vi.policy(), r["pi"])
    np.testing.assert_array_equal(vi.grid_sweeps(), r["grid_sweeps"])
    if values_t:
        np.testing.assert_array_equal(vi.values_t(), r["Vt"])
    else:
        with pytest.raises(ValueError, match="V_t"):
            vi.values_t()


def horizon_cases(cells, model, B, combos, Hs=(1, 2, 3, 7)):
    S = mg.dp.n_states(model, cells.shape[2], cells.shape[1])
    seed = 0
    for kw in combos:
        for H in Hs:
            full = dict(kw, horizon=H, gamma=kw.get("gamma", 0.95))
            vi = handle(cells, model, **full)
            ref = PolicyOptsRef(MODEL_ID[model], cells, **ref_kw(full))
            for rows in (1, H):
                for values_t in (False, True):
                    seed += 1
                    check_horizon(vi, ref, random_policy(rows, B, S, model, seed), values_t)
            vi.close()


XYD_COMBOS = [dict(dtype=d, slip_p=s, **nd) for d in ("f32", "f64") for s in (None, 0.9)
              for nd in ({}, {"lava": "nodeath", "death_cost": -0.25})]


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("env_id", ["MiniGrid-LavaGapS5-v0", "MiniGrid-LavaCrossingS9N2-v0", "MiniGrid-Empty-16x16-v0"])
def test_horizon_xyd_matches_the_restatement(env_id, B):
    horizon_cases(envs(env_id, B)[3], "xyd", B, XYD_COMBOS)


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("env_id", ["MiniGrid-DoorKey-5x5-v0", "MiniGrid-DoorKey-8x8-v0"])
def test_horizon_doorkey_matches_the_restatement(env_id, B):
    horizon_cases(envs(env_id, B)[3], "doorkey", B, [dict(dtype="f32"), dict(dtype="f64", gamma=1.0)])


def test_horizon_1024_cells():
    cells = room32()
    horizon_cases(cells, "xyd", 3, [dict(dtype="f32"), dict(dtype="f32", lava="nodeath", death_cost=-0.25, slip_p=0.9)],
                  Hs=(8,))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("env_id,model,nd", [("MiniGrid-LavaGapS5-v0", "xyd", False), ("MiniGrid-LavaGapS5-v0", "xyd", True),
                                              ("MiniGrid-LavaCrossingS9N2-v0", "xyd", True),
                                              ("MiniGrid-DoorKey-5x5-v0", "doorkey", False)])
def test_own_pi_t_over_the_envs_max_steps_reproduces_the_solve(env_id, model, nd, dtype):
    """evaluate_opts_device(None, T=H) of pi_t* after solve() equals values() of the solve bit for bit, equals
    the restatement (V_t included), and solve() afterwards is unchanged."""
    B = 3
    enc, agent, env, cells = envs(env_id, B)
    H = env.max_steps
    kw = dict(dtype=dtype, gamma=0.99, horizon=H, **({"lava": "nodeath", "death_cost": -0.05} if nd else {}))
    vi = handle(cells, model, keep_policy_t=True, **kw)
    vi.solve()
    V, pi, pit, dv = vi.values(), vi.policy(), vi.policy_t(), vi.dv
    assert vi.evaluate_opts_device(None, T=H) == H and vi.converged and vi.dv == dv
    np.testing.assert_array_equal(vi.values(), V)
    np.testing.assert_array_equal(vi.policy(), pi)
    np.testing.assert_array_equal(vi.grid_sweeps(), np.full(B, H, np.int32))
    np.testing.assert_array_equal(vi.policy_t(), pit)  # the handle's own pi_t is only read
    check_horizon(vi, PolicyOptsRef(MODEL_ID[model], cells, **ref_kw(kw)), pit, True)
    np.testing.assert_array_equal(vi.values_t()[0], V)
    with pytest.raises(ValueError, match="reset"):  # the evaluation owns the protocol state
        vi.run_local()
    vi.solve()
    np.testing.assert_array_equal(vi.values(), V)
    np.testing.assert_array_equal(vi.policy_t(), pit)
    vi.close()


def test_torch_policy_in_and_values_t_out():
    import torch

    B, H = 3, 7
    cells = envs("MiniGrid-LavaCrossingS9N2-v0", B)[3]
    kw = dict(dtype="f32", gamma=0.95, horizon=H, slip_p=0.9)
    vi = handle(cells, "xyd", **kw)
    pol = random_policy(H, B, vi.S, "xyd", 5)
    r = PolicyOptsRef(0, cells, **ref_kw(kw)).evaluate_horizon(pol)
    d_pi = torch.from_numpy(pol).cuda()
    d_vt = torch.full((H, B, vi.S), float("nan"), dtype=torch.float32, device="cuda")
    assert vi.evaluate_opts_device(d_pi.data_ptr(), T=H, values_t_ptr=d_vt.data_ptr()) == H
    vi.synchronize()
    np.testing.assert_array_equal(d_vt.cpu().numpy(), r["Vt"])
    np.testing.assert_array_equal(vi.values(), r["V"])
    np.testing.assert_array_equal(vi.policy(), r["pi"])
    # stationary, from the handle's own pi buffer: the pi_0 the call above left there
    assert vi.evaluate_opts_device(None, T=1) == H
    np.testing.assert_array_equal(vi.values(), PolicyOptsRef(0, cells, **ref_kw(kw)).evaluate_horizon(r["pi"])["V"])
    vi.close()


# ------------------------------------------------------------------------------------------------
# NoDeath, horizon 0
# ------------------------------------------------------------------------------------------------
def check_discounted(vi, ref, pol, max_sweeps=10000):
    r = ref.evaluate(pol, max_sweeps=max_sweeps)
    k = vi.evaluate_opts(pol)
    assert k == vi.sweeps == r["sweeps"] and vi.converged == r["converged"] and vi.dv == r["dv"]
    np.testing.assert_array_equal(vi.values(), r["V"])
    np.testing.assert_array_equal(vi.policy(), r["pi"])
    np.testing.assert_array_equal(vi.grid_sweeps(), r["grid_sweeps"])
    return r


@pytest.mark.parametrize("slip", [None, 0.9])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("env_id", ["MiniGrid-LavaGapS5-v0", "MiniGrid-LavaCrossingS9N2-v0", "MiniGrid-Empty-16x16-v0"])
def test_nodeath_discounted_evaluation_improvement_and_policy_iteration(env_id, dtype, slip):
    B = 3
    cells = envs(env_id, B)[3]
    kw = dict(dtype=dtype, slip_p=slip, lava="nodeath", death_cost=-0.25, gamma=0.9)
    vi = handle(cells, "xyd", **kw)
    ref = PolicyOptsRef(0, cells, **ref_kw(kw))
    pol = random_policy(1, B, vi.S, "xyd", 11)
    r = check_discounted(vi, ref, pol)
    if "Lava" in env_id:
        assert r["V"].min() < 0
    new, changed = ref.improve(r["V"], r["pi"])
    assert vi.improve_opts() == changed and changed > 0
    np.testing.assert_array_equal(vi.policy(), new)
    check_discounted(vi, ref, np.full((B, vi.S), 2, np.int8))  # all forward: into the lava for ever
    for pi0 in (None, pol):
        p = ref.policy_iteration(pi0)
        out = vi.policy_iteration_opts(pi0)
        assert (out["iters"], out["eval_sweeps"], out["changed"], out["dv"]) == (p["iters"], p["eval_sweeps"], 0, p["dv"])
        assert vi.sweeps == p["sweeps"]
        np.testing.assert_array_equal(vi.values(), p["V"])
        np.testing.assert_array_equal(vi.policy(), p["pi"])
        np.testing.assert_array_equal(vi.grid_sweeps(), p["grid_sweeps"])
    one = vi.policy_iteration_opts(pol, max_iters=1)
    assert one["iters"] == 1 and one["changed"] == ref.policy_iteration(pol, max_iters=1)["changed"] > 0
    vi.solve()  # the solve resets and behaves as before
    vi.close()


def test_nodeath_discounted_1024_cells_and_a_sweep_cap():
    cells = room32()
    kw = dict(dtype="f32", lava="nodeath", death_cost=-0.25, gamma=0.9)
    vi = handle(cells, "xyd", **kw)
    check_discounted(vi, PolicyOptsRef(0, cells, **ref_kw(kw)), random_policy(1, 3, vi.S, "xyd", 3))
    vi.close()
    vi = handle(cells, "xyd", max_sweeps=5, **kw)
    r = check_discounted(vi, PolicyOptsRef(0, cells, **ref_kw(kw)), np.full((3, vi.S), 2, np.int8), max_sweeps=5)
    assert not r["converged"] and not vi.converged and vi.sweeps == 5
    vi.close()


def test_nodeath_discounted_batch_past_the_in_kernel_reduction():
    B = 513
    cells = envs("MiniGrid-LavaGapS5-v0", B)[3]
    kw = dict(dtype="f32", lava="nodeath", death_cost=-0.25, gamma=0.9, slip_p=0.9)
    vi = handle(cells, "xyd", **kw)
    check_discounted(vi, PolicyOptsRef(0, cells, **ref_kw(kw)), random_policy(1, B, vi.S, "xyd", 4))
    vi.close()
    hk = dict(dtype="f32", gamma=0.95, horizon=3)
    vi = handle(cells, "xyd", **hk)
    check_horizon(vi, PolicyOptsRef(0, cells, **ref_kw(hk)), random_policy(3, B, vi.S, "xyd", 6), True)
    vi.close()


# ------------------------------------------------------------------------------------------------
# Ties to the env on the device: gamma = 1, fp64, no slip -- rollout() collects V_0[start]
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,model,dc", [("MiniGrid-LavaCrossingS9N2-v0", "xyd", None),
                                             ("MiniGrid-LavaCrossingS9N2-v0", "xyd", -0.01),
                                             ("MiniGrid-LavaCrossingS9N2-v0", "xyd", -0.3),
                                             ("MiniGrid-DoorKey-6x6-v0", "doorkey", None)])
def test_rollout_collects_v0_of_the_evaluated_policy(env_id, model, dc):
    B, H = 6, 48
    enc, agent, env, cells = envs(env_id, B)
    nd = dc is not None
    kw = dict(dtype="f64", gamma=1.0, horizon=H, **({"lava": "nodeath", "death_cost": dc} if nd else {}))
    vi = handle(cells, model, keep_policy_t=True, **kw)
    vi.solve()
    pit = vi.policy_t()
    third = pit.copy()
    third[::3][third[::3] >= 0] = 2
    pols = {"pi_t*": pit, "noisy_t": rr.noisy_policy(pit[0], model, 0.3, T=H), "noisy": rr.noisy_policy(pit[0], model, 0.3),
            "forward": np.where(pit[0] >= 0, 2, -1).astype(np.int8), "third_forward": third}
    venv = mg.MiniGridVecEnv(env_id, B, **({"no_death_types": ("lava",), "death_cost": dc} if nd else {}))
    start = rr.start_states(enc, agent, model)
    bound = H * 2.0 ** -52 * (H * abs(dc or 0.0) + 1.0)  # tests/test_policy_opts_cpu.py: opposite summation orders
    entered = snap_exact = snap_lava = False
    for name, pol in pols.items():
        vi.evaluate_opts(pol, values_t=True)
        v0 = vi.values()[np.arange(B), start]
        venv.load(enc, agent, max_steps=H)
        res = venv.rollout(pol, model=model)
        assert res.ok, name
        # lava entries per env, from the host rollout's trace (tests/test_policy_opts_cpu.py)
        m = np.zeros(B, np.int64)
        if nd:
            ro = rr.rollout_ref(enc, agent, pol, model, H, env.see_through_walls, trace_len=H, nd_types=("lava",),
                                death_cost=dc)
            np.testing.assert_array_equal(res.ret, ro["ret"])
            m = lava_entries(ro, cells, enc.shape[1])
            entered |= bool((m >= 1).any())
        exact = m == 0  # at most one non-zero reward collected
        np.testing.assert_array_equal(res.ret[exact], v0[exact], err_msg=name)
        assert (np.abs(res.ret - v0)[~exact] <= bound).all(), name
        if model == "xyd":
            # a non-reset snapshot: 7 steps in, the rest of the episode collects V_7 at the state reached --
            # exactly where it enters no lava from there on, within the bound where it does
            venv.load(enc, agent, max_steps=H)
            first = venv.rollout(pol, model=model, max_steps=7)
            st = venv.get_state()
            run = ~(first.terminated | first.truncated)
            assert run.any() and (st["step_count"][run] == 7).all(), name
            rest = venv.rollout(pol, model=model)
            s7 = np.array([state_index(model, venv.W, *(int(v) for v in st["agent"][b])) for b in range(B)])
            v7 = vi.values_t()[7][np.arange(B), s7]
            m7 = lava_entries(ro, cells, enc.shape[1], first=7) if nd else m
            np.testing.assert_array_equal(rest.ret[run & (m7 == 0)], v7[run & (m7 == 0)], err_msg=name)
            assert (np.abs(rest.ret - v7)[run & (m7 >= 1)] <= bound).all(), name
            snap_exact |= bool((run & (m7 == 0)).any())
            snap_lava |= bool((run & (m7 >= 1)).any())
    if model == "xyd":
        assert snap_exact, "no snapshot collected a lava-free rest of an episode"
    if nd:
        assert snap_lava, "no NoDeath snapshot entered lava after step 7"
        assert entered, "the NoDeath case needs a policy that walks into the lava"
    venv.close()
    vi.close()


def test_slip_rollouts_average_to_v0():
    """A sanity run, not the parity check: 4096 slip rollouts of pi_t* on one grid average to V_0[start]
    within 5 standard errors (seed 0: the host restatement's rollouts satisfy the same bound)."""
    B, p, H = 4096, 0.9, 64  # (H = 64, not the env's 324: the replicated pi_t stays under 100 MB)
    enc1, agent1, env, cells1 = envs("MiniGrid-LavaCrossingS9N1-v0", 1)
    vi = handle(cells1, "xyd", dtype="f64", gamma=1.0, horizon=H, slip_p=p, keep_policy_t=True)
    vi.solve()
    pit = vi.policy_t()
    assert vi.evaluate_opts_device(None, T=H) == H
    v0 = vi.values()[0, rr.start_states(enc1, agent1, "xyd")[0]]
    vi.close()
    venv = mg.MiniGridVecEnv("MiniGrid-LavaCrossingS9N1-v0", B)
    venv.load(np.repeat(enc1, B, axis=0), np.repeat(agent1, B, axis=0), max_steps=H)
    venv.set_slip(p, seed=0)
    res = venv.rollout(np.ascontiguousarray(np.repeat(pit, B, axis=1)), model="xyd")
    venv.close()
    assert res.ok and abs(res.ret.mean() - v0) <= 5 * res.ret.std() / np.sqrt(B), (res.ret.mean(), v0, res.ret.std())


# ------------------------------------------------------------------------------------------------
# Refusals, and the plain handle
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    B, H = 3, 6
    cells = envs("MiniGrid-LavaGapS5-v0", B)[3]
    kw = dict(dtype="f32", gamma=0.95, horizon=H)
    vi = handle(cells, "xyd", **kw)
    ref = PolicyOptsRef(0, cells, **ref_kw(kw))
    S = vi.S
    for T in (2, 5, 7):
        with pytest.raises(ValueError, match="shape"):
            vi.evaluate_opts(np.zeros((T, B, S), np.int8))
        with pytest.raises(ValueError, match="T ="):
            vi.evaluate_opts_device(None, T=T)
    with pytest.raises(ValueError, match="MGDP_KEEP_POLICY_T"):
        vi.evaluate_opts_device(None, T=H)
    with pytest.raises(ValueError, match="finite horizon"):
        vi.improve_opts()
    with pytest.raises(ValueError, match="finite horizon"):
        vi.policy_iteration_opts()
    for fn in (vi.evaluate, vi.evaluate_device, vi.improve, vi.policy_iteration):  # the old names keep refusing
        with pytest.raises(ValueError):
            fn(*((np.zeros((B, S), np.int8),) if fn == vi.evaluate else ()))
    # the bad-lane message: the lowest grid, its largest t, that row's lowest state
    v1 = np.nonzero(~ref.absorb[1])[0]
    v2 = np.nonzero(~ref.absorb[2])[0]
    pi = random_policy(H, B, S, "xyd", 8)
    pi[1, 1, v1[3]] = 7
    pi[4, 1, v1[5]] = -1
    pi[4, 1, v1[9]] = 9
    pi[5, 2, v2[0]] = 7
    with pytest.raises(ValueError, match=f"grid 1 t 4 state {v1[5]}: action -1 is outside \\[0, 7\\)") as e:
        vi.evaluate_opts(pi, values_t=True)
    with pytest.raises(ValueError) as e_ref:
        ref.evaluate_horizon(pi)
    assert str(e.value) == str(e_ref.value)
    stat = random_policy(1, B, S, "xyd", 9)
    stat[2, v2[4]] = 7
    with pytest.raises(ValueError, match=f"grid 2 t 0 state {v2[4]}: action 7 "):
        vi.evaluate_opts(stat)
    check_horizon(vi, ref, random_policy(H, B, S, "xyd", 10), True)  # a working call afterwards
    vi.close()
    # horizon 0: T must be 1, no V_t; DoorKey bad lane
    nd = handle(cells, "xyd", lava="nodeath")
    with pytest.raises(ValueError, match="shape"):
        nd.evaluate_opts(np.zeros((H, B, S), np.int8))
    with pytest.raises(ValueError, match="finite horizon"):
        nd.evaluate_opts(np.zeros((B, S), np.int8), values_t=True)
    with pytest.raises(ValueError, match="T ="):
        nd.evaluate_opts_device(None, T=H)
    bad = np.full((B, S), 2, np.int8)
    s = int(np.nonzero(~PolicyOptsRef(0, cells, lava="nodeath").absorb[1])[0][2])
    bad[1, s] = 7
    with pytest.raises(ValueError, match=f"grid 1 state {s}: action 7 "):
        nd.evaluate_opts(bad)
    nd.evaluate_opts(np.full((B, S), 2, np.int8))
    nd.close()
    dk = envs("MiniGrid-DoorKey-5x5-v0", 3)[3]
    hd = handle(dk, "doorkey", horizon=4, gamma=1.0)
    dref = PolicyOptsRef(1, dk, gamma=1.0, horizon=4)
    pi = random_policy(4, 3, hd.S, "doorkey", 12)
    vs = np.nonzero(~dref.absorb[0])[0]
    pi[2, 0, vs[-1]] = 5
    pi[2, 0, vs[7]] = 6
    with pytest.raises(ValueError, match=f"grid 0 t 2 state {vs[7]}: action 6 is outside \\[0, 5\\)"):
        hd.evaluate_opts(pi)
    hd.close()


@pytest.mark.parametrize("env_id,B", [("MiniGrid-LavaCrossingS9N2-v0", 3), ("MiniGrid-Empty-16x16-v0", 2)])
@pytest.mark.parametrize("t_bad", [5, 4, 0])
def test_bad_lanes_in_several_waves_name_the_rows_lowest_state(env_id, B, t_bad):
    """Offending states of one row in different waves of the workgroup (81 cells: two waves, 256: four):
    the message names the lowest of them whichever wave gets there first, every wave stops at the same
    sweep, and the handle works afterwards.  H = 9: sweep H-1-t_bad is the last slot of a prefetch round
    (t_bad = 5), the first (4), and the very last sweep (0); a lower row holds a still lower bad state."""
    H = 9
    cells = envs(env_id, B)[3]
    kw = dict(dtype="f32", gamma=0.95, horizon=H)
    vi = handle(cells, "xyd", **kw)
    ref = PolicyOptsRef(0, cells, **ref_kw(kw))
    g = B - 1
    valid = np.nonzero(~ref.absorb[g])[0]
    waves = valid // 4 // 64  # the wave of each valid state's cell
    assert waves.max() >= 1
    pi = random_policy(H, B, vi.S, "xyd", 20 + t_bad)
    picks = [int(valid[waves == w][1 if w == 0 else -1]) for w in range(int(waves.max()) + 1) if (waves == w).any()]
    for s in picks:
        pi[t_bad, g, s] = 7
    if t_bad > 0:
        pi[t_bad - 1, g, valid[0]] = 7  # a row the induction never reaches
    with pytest.raises(ValueError) as e_ref:
        ref.evaluate_horizon(pi)
    assert f"grid {g} t {t_bad} state {min(picks)}: action 7 " in str(e_ref.value)
    for values_t in (False, True, False, True, False):
        with pytest.raises(ValueError) as e:
            vi.evaluate_opts(pi, values_t=values_t)
        assert str(e.value) == str(e_ref.value)
    check_horizon(vi, ref, random_policy(H, B, vi.S, "xyd", 30), True)
    vi.close()


@pytest.mark.parametrize("model,env_id,slip", [("xyd", "MiniGrid-LavaCrossingS9N2-v0", None),
                                               ("xyd", "MiniGrid-LavaCrossingS9N2-v0", 0.9),
                                               ("doorkey", "MiniGrid-DoorKey-5x5-v0", None)])
def test_plain_handle_gives_the_plain_results(model, env_id, slip):
    B = 3
    cells = envs(env_id, B)[3]
    vi = handle(cells, model, dtype="f32", slip_p=slip)
    pol = random_policy(1, B, vi.S, model, 13)
    k = vi.evaluate(pol)
    V, pi, gs, dv = vi.values(), vi.policy(), vi.grid_sweeps(), vi.dv
    assert vi.evaluate_opts(pol) == k and vi.dv == dv
    np.testing.assert_array_equal(vi.values(), V)
    np.testing.assert_array_equal(vi.policy(), pi)
    np.testing.assert_array_equal(vi.grid_sweeps(), gs)
    assert vi.evaluate_opts_device(None) == k
    np.testing.assert_array_equal(vi.values(), V)
    n = vi.improve_opts()
    pi2 = vi.policy()
    vi.evaluate(pol)
    assert vi.improve() == n
    np.testing.assert_array_equal(vi.policy(), pi2)
    a, b = vi.policy_iteration_opts(pol, max_iters=3), None
    Va = vi.values()
    b = vi.policy_iteration(pol, max_iters=3)
    assert a == b
    np.testing.assert_array_equal(vi.values(), Va)
    with pytest.raises(ValueError, match="finite horizon"):
        vi.evaluate_opts(pol, values_t=True)
    vi.close()


@functools.lru_cache(maxsize=None)
def room40():
    """Two 40 x 40 rooms, 1600 cells each: above the option kernels' 1024, so the evaluation is the strided
    form of vi_eval_kernel (about 51 KiB of LDS in fp32).  One empty with a goal; one with a few walls and
    a lava cell before its goal."""
    out = []
    for b in range(2):
        c = np.full((40, 40), 1, np.uint8)
        c[0, :] = c[-1, :] = c[:, 0] = c[:, -1] = 2
        c[38, 38] = 8
        if b:
            c[12, 1:30] = 2
            c[25, 8:39] = 2
            c[5:20, 33] = 2
            c[37, 30] = 9
        out.append(c)
    return np.stack(out)


def test_plain_handle_above_1024_cells_is_the_same_through_both_families():
    """A plain handle is not bound by the option handles' W*H <= 1024: the *_opts names reach the same
    strided evaluation as the plain names, result for result, and both match the restatement bit for bit."""
    cells, B = room40(), 2
    vi = handle(cells, "xyd", dtype="f32", gamma=0.99)
    ref = PolicyRef(0, cells, gamma=0.99, dtype="f32")
    # pi* with a seeded 2 % of the lanes replaced: most states still reach the goal, later and on other paths
    # (V != 0 on thousands of states, 128 sweeps, the two grids stop at different sweeps)
    rng = np.random.default_rng(40)
    pol = oracle.value_iteration(0, cells, dtype="f32", gamma=0.99)["pi"].copy()
    swap = rng.random((B, vi.S)) < 0.02
    pol[swap] = rng.integers(0, n_actions("xyd"), int(swap.sum()))
    r = ref.evaluate(pol)

    def state():
        return vi.values(), vi.policy(), vi.grid_sweeps(), vi.sweeps, vi.dv

    def same(a, b):
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
        assert a[3:] == b[3:]

    want = (r["V"], r["pi"], r["grid_sweeps"], r["sweeps"], r["dv"])
    for fn in (vi.evaluate, vi.evaluate_opts):
        assert fn(pol) == r["sweeps"] and vi.converged == r["converged"]
        same(state(), want)
    for fn in (vi.evaluate_device, vi.evaluate_opts_device):  # the handle's own buffer: pol, normalised
        assert fn(None) == r["sweeps"]
        same(state(), want)
    got = []
    for fn in (vi.improve, vi.improve_opts):
        vi.evaluate(pol)
        got.append((fn(), state()))
    assert got[0][0] == got[1][0] > 0
    same(got[0][1], got[1][1])
    got = [(fn(pol, max_iters=3), state()) for fn in (vi.policy_iteration, vi.policy_iteration_opts)]
    assert got[0][0] == got[1][0]
    same(got[0][1], got[1][1])
    vi.close()


def test_module_helpers_route_to_the_opts_entry_points():
    B, H = 3, 5
    cells = envs("MiniGrid-LavaGapS5-v0", B)[3]
    S = mg.dp.n_states("xyd", 5, 5)
    pol = random_policy(H, B, S, "xyd", 14)
    r = mg.policy_evaluation(cells, pol, model="xyd", horizon=H, gamma=1.0, dtype="f64")
    np.testing.assert_array_equal(r.V, PolicyOptsRef(0, cells, gamma=1.0, dtype="f64", horizon=H).evaluate_horizon(pol)["V"])
    p = PolicyOptsRef(0, cells, lava="nodeath", death_cost=-0.25, dtype="f64").policy_iteration()
    r = mg.policy_iteration(cells, model="xyd", lava="nodeath", death_cost=-0.25, dtype="f64")
    assert (r.iters, r.changed) == (p["iters"], 0)
    np.testing.assert_array_equal(r.V, p["V"])
