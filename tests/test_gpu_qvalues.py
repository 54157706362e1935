"""Action values on the GPU (vi_qvalues_kernel) against the numpy restatement
tests/qvalues_ref.py applied to the handle's own values(): Q and opt array-equal, signed zeros included.  values()
is pinned to the oracle once per shape.

Shapes: Empty-5x5 (25 cells: idle lanes in the only wave), a served lone Empty-16x16, FourRooms (361 cells over
a 256-thread workgroup: the strided item loop, several waves' pieces), 65 LavaCrossingS9N1 grids under NoDeath
(grid offsets past one wave of grids, negative Q), DoorKey 5x5 and 8x8 (the 20-value item of a DoorKey
direction), and the grids over 1024 cells of tests/test_gpu_large_grids.py up to the largest LDS layouts.
"""
import functools

import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from minigrid_dynamicprogramming_amd import _lib
from oracle import oracle
from tests import qlearn_ref as qr
from tests import qvalues_ref as qv
from tests import rollout_ref as rr
from tests.test_gpu_large_grids import _cells as large_cells
from tests.test_gpu_large_grids import _doorkey33, _ref as large_ref

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
NP = {"f32": np.float32, "f64": np.float64}
A_OF = {"xyd": 7, "doorkey": 5}


@functools.lru_cache(maxsize=None)
def grids(env_id, B):
    return rr.cells_of(rr.grids(env_id, B)[0])


def random_policy(ref, seed):
    return np.random.default_rng(seed).integers(0, ref.A, (ref.B, ref.S)).astype(np.int8)


def check_q(vi, ref, oracle_V=None):
    """Q and opt of the handle against the restatement on the handle's own V; returns them."""
    V = vi.values()
    if oracle_V is not None:
        np.testing.assert_array_equal(V, oracle_V)
    want_q, want_opt = qv.q_and_opt(ref, V)
    Q, opt = vi.action_values(optimal=True)
    assert Q.dtype == vi.np_dtype and Q.shape == (vi.B, vi.S, A_OF[vi.model]) and Q.shape[2] == ref.A
    assert opt.dtype == np.uint8 and opt.shape == (vi.B, vi.S)
    np.testing.assert_array_equal(Q, want_q)
    np.testing.assert_array_equal(np.signbit(Q), np.signbit(want_q))
    np.testing.assert_array_equal(opt, want_opt)
    assert not Q[ref.absorb].any() and not opt[ref.absorb].any() and (opt[~ref.absorb] != 0).all()
    return Q, opt


def snapshot(vi):
    return vi.values(), vi.policy(), vi.sweeps, vi.dv, vi.converged, vi.grid_sweeps()


def assert_same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty5_idle_lanes_in_the_only_wave(dtype):
    cells = grids("MiniGrid-Empty-5x5-v0", 3)
    o = oracle.value_iteration(0, cells, dtype=dtype, fixed_point=True)
    vi = mg.ValueIteration(cells, dtype=dtype)
    try:
        vi.solve()
        check_q(vi, qv.make_ref(0, cells, dtype=dtype), o["V"])
    finally:
        vi.close()


def test_served_lone_grid_leaves_and_is_served_again():
    """The server leaves, V is in HBM; a following solve() is served again and gives the same bits."""
    cells = grids("MiniGrid-Empty-16x16-v0", 1)
    o = oracle.value_iteration(0, cells, dtype="f32", fixed_point=True)
    vi = mg.ValueIteration(cells, dtype="f32")
    try:
        assert vi.persistent
        name = vi.kernel_name
        k = vi.solve()
        Q, opt = check_q(vi, qv.make_ref(0, cells, dtype="f32"), o["V"])
        assert vi.persistent and vi.kernel_name == name
        assert vi.solve() == k == o["sweeps"] and vi.dv == o["dv"]
        np.testing.assert_array_equal(vi.values(), o["V"])
        np.testing.assert_array_equal(vi.policy(), o["pi"])
        Q2, opt2 = vi.action_values(optimal=True)
        np.testing.assert_array_equal(Q2, Q)
        np.testing.assert_array_equal(opt2, opt)
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slip", [None, 0.9])
def test_fourrooms_strided_items(slip, dtype):
    cells = grids("MiniGrid-FourRooms-v0", 3)
    o = oracle.value_iteration(0, cells, slip_p=slip, dtype=dtype)
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip)
    try:
        vi.solve()
        check_q(vi, qv.make_ref(0, cells, slip_p=slip, dtype=dtype), o["V"])
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slip", [None, 0.9])
def test_nodeath_lava_65_grids_negative_q(slip, dtype):
    cells = grids("MiniGrid-LavaCrossingS9N1-v0", 65)
    o = oracle.value_iteration_ex(0, cells, slip_p=slip, dtype=dtype, lava_mode=1, death_cost=-1.0)
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip, lava="nodeath", death_cost=-1.0)
    try:
        vi.solve()
        Q, _ = check_q(vi, qv.make_ref(0, cells, slip_p=slip, dtype=dtype, lava="nodeath", death_cost=-1.0), o["V"])
        assert Q.min() < 0 and (Q[64] != 0).any()
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [5, 8])
def test_doorkey_items(size, dtype):
    cells = grids(f"MiniGrid-DoorKey-{size}x{size}-v0", 3)
    o = oracle.value_iteration(1, cells, dtype=dtype, fixed_point=True)
    vi = mg.ValueIteration(cells, model="doorkey", dtype=dtype)
    try:
        vi.solve()
        Q, opt = check_q(vi, qv.make_ref(1, cells, dtype=dtype), o["V"])
        assert (opt < 32).all() and ((opt & 24) != 0).any()  # five lanes; pickup / toggle are optimal somewhere
    finally:
        vi.close()


@pytest.mark.parametrize("W,H,B,dtype", [(33, 33, 3, "f32"), (33, 33, 3, "f64"), (9, 130, 3, "f32"), (66, 66, 1, "f32")])
def test_xyd_over_1024_cells(W, H, B, dtype):
    cells = large_cells(W, H, B)
    o = large_ref(W, H, B, dtype, None)
    vi = mg.ValueIteration(cells, dtype=dtype)
    try:
        vi.solve()
        Q, _ = check_q(vi, qv.make_ref(0, cells, dtype=dtype), o["V"])
        assert (Q.reshape(B, W * H, 28)[:, 1024:] > 0).any()  # the cells past the first 1024 matter
    finally:
        vi.close()


def test_doorkey_33x33():
    cells = _doorkey33()[1:2]
    o = oracle.value_iteration(1, cells, dtype="f32", fixed_point=True)
    vi = mg.ValueIteration(cells, model="doorkey", dtype="f32")
    try:
        vi.solve()
        Q, _ = check_q(vi, qv.make_ref(1, cells, dtype="f32"), o["V"])
        assert (Q.reshape(1, 33 * 33, 80)[:, 1024:] > 0).any()
    finally:
        vi.close()


# ------------------------------------------------------------------------------------------------ behaviour
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slip", [None, 0.9])
def test_q_pi_after_evaluating_a_random_policy(slip, dtype):
    cells = grids("MiniGrid-FourRooms-v0", 3)
    ref = qv.make_ref(0, cells, slip_p=slip, dtype=dtype)
    pi = random_policy(ref, 11)
    vi = mg.ValueIteration(cells, dtype=dtype, slip_p=slip)
    try:
        vi.evaluate(pi)
        r = ref.evaluate(pi)
        Q, _ = check_q(vi, ref, r["V"])
        # Q^pi[s, pi(s)] is one more sweep of the evaluation
        valid = ~ref.absorb
        Vn, _ = ref.sweep(r["V"], r["pi"])
        got = np.take_along_axis(Q, np.clip(r["pi"], 0, 6).astype(np.int64)[..., None], axis=2)[..., 0]
        np.testing.assert_array_equal(got[valid], Vn[valid])
    finally:
        vi.close()


def test_q_after_policy_iteration_on_a_nodeath_handle():
    cells = grids("MiniGrid-LavaCrossingS9N1-v0", 3)
    ref = qv.make_ref(0, cells, dtype="f64", lava="nodeath", death_cost=-1.0)
    r = ref.policy_iteration(np.full((3, ref.S), 2, np.int8))
    vi = mg.ValueIteration(cells, dtype="f64", lava="nodeath", death_cost=-1.0)
    try:
        vi.policy_iteration_opts()
        Q, opt = check_q(vi, ref, r["V"])
        assert Q.min() < 0
        assert vi.is_optimal(vi.policy()).all()  # the stable policy is greedy on its own V
    finally:
        vi.close()


def test_q_only_opt_only_and_both_give_the_same_bits():
    cells = grids("MiniGrid-DoorKey-8x8-v0", 3)
    vi = mg.ValueIteration(cells, model="doorkey", dtype="f32")
    try:
        vi.solve()
        Q, opt = vi.action_values(optimal=True)
        np.testing.assert_array_equal(vi.action_values(), Q)
        np.testing.assert_array_equal(vi.optimal_actions(), opt)
        L = _lib.load()
        assert L.mgdp_vi_action_values(vi.h, None, None) == _lib.MGDP_E_INVALID
        assert L.mgdp_vi_action_values_device(vi.h, None, None) == _lib.MGDP_E_INVALID
        with pytest.raises(ValueError, match="both outputs are null"):
            vi.action_values_device(None, None)
    finally:
        vi.close()


def test_refusals():
    cells = grids("MiniGrid-Empty-5x5-v0", 3)
    vi = mg.ValueIteration(cells)
    try:
        for call in (vi.action_values, vi.optimal_actions):
            with pytest.raises(ValueError, match="no value function"):
                call()
        with pytest.raises(ValueError, match="no value function"):
            vi.improve()
    finally:
        vi.close()
    vi = mg.ValueIteration(cells, horizon=20)
    try:
        vi.solve()
        with pytest.raises(ValueError, match="refused on a finite horizon: Q_t needs V_\\{t\\+1\\}"):
            vi.action_values()
        assert _lib.load().mgdp_vi_action_values(vi.h, None, _lib.ptr(np.empty((3, 100), np.uint8))) == _lib.MGDP_E_UNSUPPORTED
    finally:
        vi.close()
    vi = mg.ValueIteration(cells, method="sweep")
    try:
        vi.solve()
        with pytest.raises(ValueError, match="fused method only"):
            vi.improve()
        with pytest.raises(ValueError, match="fused method only"):
            vi.action_values()
    finally:
        vi.close()


def test_device_entry_on_torch_tensors_and_alignment():
    import torch

    cells = grids("MiniGrid-FourRooms-v0", 3)
    vi = mg.ValueIteration(cells, dtype="f64", slip_p=0.9)
    try:
        vi.solve()
        want_q, want_opt = vi.action_values(optimal=True)
        Q = torch.full((3, vi.S, 7), -7.0, dtype=torch.float64, device="cuda")
        opt = torch.full((3, vi.S), 255, dtype=torch.uint8, device="cuda")
        vi.action_values_device(Q.data_ptr(), opt.data_ptr())
        np.testing.assert_array_equal(Q.cpu().numpy(), want_q)
        np.testing.assert_array_equal(opt.cpu().numpy(), want_opt)
        Q.fill_(-7.0)
        opt.fill_(255)
        vi.action_values_device(Q.data_ptr())
        np.testing.assert_array_equal(Q.cpu().numpy(), want_q)
        assert (opt == 255).all()
        vi.action_values_device(None, opt.data_ptr())
        np.testing.assert_array_equal(opt.cpu().numpy(), want_opt)
        Q.fill_(-7.0)
        opt.fill_(255)
        for q_ptr, o_ptr in ((Q.data_ptr() + 8, opt.data_ptr()), (Q.data_ptr(), opt.data_ptr() + 4), (None, opt.data_ptr() + 1)):
            with pytest.raises(ValueError, match="16-byte aligned"):
                vi.action_values_device(q_ptr, o_ptr)
        assert (Q == -7.0).all() and (opt == 255).all()
    finally:
        vi.close()


@pytest.mark.parametrize("kw", [dict(dtype="f32"), dict(dtype="f64", slip_p=0.9)])
def test_the_call_leaves_the_handle_as_it_was(kw):
    cells = grids("MiniGrid-FourRooms-v0", 3)
    vi = mg.ValueIteration(cells, **kw)
    fresh = mg.ValueIteration(cells, **kw)
    try:
        vi.solve()
        before = snapshot(vi)
        vi.action_values(optimal=True)
        vi.optimal_actions()
        assert_same(snapshot(vi), before)
        # a later solve behaves exactly as it would have: the second solve of a handle never asked
        fresh.solve()
        fresh.solve()
        vi.solve()
        assert_same(snapshot(vi), snapshot(fresh))
        # ... and after an evaluation
        pi = random_policy(qv.make_ref(0, cells), 5)
        vi.evaluate(pi)
        before = snapshot(vi)
        vi.action_values()
        assert_same(snapshot(vi), before)
    finally:
        vi.close()
        fresh.close()


def test_kernel_time_counts_the_launch():
    cells = grids("MiniGrid-Empty-5x5-v0", 3)
    vi = mg.ValueIteration(cells)
    try:
        vi.solve()
        vi.enable_timing(True)
        vi.optimal_actions()
        vi.action_values()
        ms, n = vi.kernel_time()
        assert n == 2 and ms > 0
    finally:
        vi.close()


@pytest.mark.parametrize("model,env_id,slip", [("xyd", "MiniGrid-FourRooms-v0", None), ("xyd", "MiniGrid-FourRooms-v0", 0.9),
                                               ("doorkey", "MiniGrid-DoorKey-8x8-v0", None)])
def test_improve_changes_exactly_the_states_without_their_bit(model, env_id, slip):
    cells = grids(env_id, 3)
    mid = 0 if model == "xyd" else 1
    ref = qv.make_ref(mid, cells, slip_p=slip, dtype="f32")
    vi = mg.ValueIteration(cells, model=model, dtype="f32", slip_p=slip)
    try:
        vi.evaluate(random_policy(ref, 3))
        opt, old = vi.optimal_actions(), vi.policy()
        valid = opt != 0
        np.testing.assert_array_equal(valid, ~ref.absorb)
        changed = vi.improve()
        new = vi.policy()
        assert changed == int((valid & ~qv.lane_bit(opt, old)).sum()) and changed > 0
        assert qv.lane_bit(opt, new)[valid].all()
        np.testing.assert_array_equal(vi.is_optimal(old), ~valid | qv.lane_bit(opt, old))
    finally:
        vi.close()


@pytest.mark.parametrize("model,env_id", [("xyd", "MiniGrid-FourRooms-v0"), ("doorkey", "MiniGrid-DoorKey-8x8-v0")])
def test_is_optimal(model, env_id):
    cells = grids(env_id, 3)
    vi = mg.ValueIteration(cells, model=model, dtype="f32")
    try:
        vi.solve()
        assert vi.dv == 0.0
        pi, opt = vi.policy(), vi.optimal_actions()
        ok = vi.is_optimal(pi)
        assert ok.dtype == np.bool_ and ok.shape == pi.shape and ok.all()
        # one deliberately wrong lane: a valid state with an action outside its optimal set
        b, s = np.argwhere((opt != 0) & (opt != (1 << A_OF[model]) - 1))[0]
        wrong = int(np.nonzero(((opt[b, s] >> np.arange(A_OF[model])) & 1) == 0)[0][0])
        bad = pi.copy()
        bad[b, s] = wrong
        ok = vi.is_optimal(bad)
        assert not ok[b, s]
        ok[b, s] = True
        assert ok.all()
        # another member of a tie set is optimal too
        b, s = np.argwhere((opt & (opt - 1)) != 0)[0]
        other = pi.copy()
        other[b, s] = int(np.nonzero((opt[b, s] >> np.arange(8)) & 1)[0][-1])
        assert other[b, s] != pi[b, s] and vi.is_optimal(other).all()
        # checked as _check_policy checks
        with pytest.raises(ValueError, match="does not match"):
            vi.is_optimal(pi[:, :-4])
        with pytest.raises(ValueError, match="integer array"):
            vi.is_optimal(pi.astype(np.float32))
    finally:
        vi.close()


def test_q_greedy_of_the_table_is_the_policy():
    enc, agent, _ = rr.grids("MiniGrid-FourRooms-v0", 3)
    cells = rr.cells_of(enc)
    vi = mg.ValueIteration(cells, dtype="f64")
    venv = mg.MiniGridVecEnv("MiniGrid-FourRooms-v0", 3)
    try:
        vi.solve()
        assert vi.dv == 0.0
        Q, opt = vi.action_values(optimal=True)
        venv.load(enc, agent)
        pi, vq = venv.q_greedy(Q, values=True)
        valid = opt != 0
        np.testing.assert_array_equal(pi[valid], vi.policy()[valid])
        np.testing.assert_array_equal(vq[valid], vi.values()[valid])
    finally:
        vi.close()
        venv.close()


def test_learned_table_ties_with_the_gpu_q_star():
    """The per-(s, a) tie of tests/test_qvalues_cpu.py with both sides from the GPU."""
    c = qr.tie_case("empty5_a3")
    cells = rr.cells_of(c["enc"])
    assert cells.shape[0] == 8
    venv = mg.MiniGridVecEnv(c["env_id"], 8)
    vi = mg.ValueIteration(cells, gamma=qr.TIE_GAMMA, tol=1e-13, dtype="f64")
    try:
        venv.load(c["enc"], c["agent"])
        res = venv.q_learn(c["n_steps"], model="xyd", alpha=1.0, gamma=qr.TIE_GAMMA, eps=1.0, n_act=3, unit_goal=True, seed=0)
        vi.solve()
        np.testing.assert_array_equal(vi.values(), c["V"])
        Q = vi.action_values()
        on = c["V"] > 0
        err = float(np.abs(res.Q[..., :3] - Q[..., :3])[on].max())
        print(f"empty5_a3: max |Q_learn - Q*| = {err:.3e}")
        assert err <= qr.TIE_TOL
    finally:
        vi.close()
        venv.close()


def test_module_level_action_values():
    cells = grids("MiniGrid-LavaCrossingS9N1-v0", 3)
    r = mg.action_values(cells, dtype="f64")
    assert isinstance(r, mg.ActionValues) and r.model == "xyd" and r.sweeps > 0
    ref = qv.make_ref(0, cells, dtype="f64")
    want_q, want_opt = qv.q_and_opt(ref, r.V)
    np.testing.assert_array_equal(r.Q, want_q)
    np.testing.assert_array_equal(r.opt, want_opt)
    adv = r.advantage()
    valid = ~ref.absorb
    assert (adv <= 0).all() and (adv.max(-1)[valid] == 0).all() and not adv[ref.absorb].any()
    # a given policy on an option handle goes through evaluate_opts
    refn = qv.make_ref(0, cells, dtype="f64", lava="nodeath")
    pi = random_policy(refn, 2)
    r = mg.action_values(cells, pi=pi, dtype="f64", lava="nodeath")
    np.testing.assert_array_equal(r.V, refn.evaluate(pi)["V"])
    np.testing.assert_array_equal(r.Q, qv.q_table(refn, r.V))
    np.testing.assert_array_equal(r.pi, refn.normalise(pi))
