"""Action values: facts of the numpy restatement (tests/qvalues_ref.py) that the GPU tests of DESIGN.md
section 22 build on, and the C ABI of the new entry points.  No GPU.
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

ENVS = {"fourrooms": ("MiniGrid-FourRooms-v0", 0), "lava9": ("MiniGrid-LavaCrossingS9N1-v0", 0),
        "empty5": ("MiniGrid-Empty-5x5-v0", 0), "doorkey5": ("MiniGrid-DoorKey-5x5-v0", 1),
        "doorkey8": ("MiniGrid-DoorKey-8x8-v0", 1)}


@functools.lru_cache(maxsize=None)
def cells_of(name, B=3):
    return rr.cells_of(rr.grids(ENVS[name][0], B)[0])


def test_abi_exports_the_action_value_entry_points():
    L = _lib.load()
    for name in ("mgdp_vi_action_values", "mgdp_vi_action_values_device"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.mgdp_abi_version() == 12  # additive: the version does not move
    assert L.mgdp_vi_action_values(None, None, None) == _lib.MGDP_E_INVALID
    assert L.mgdp_vi_action_values_device(None, None, None) == _lib.MGDP_E_INVALID
    assert {"action_values", "ActionValues"} <= set(dir(mg))
    for m in ("action_values", "optimal_actions", "action_values_device", "is_optimal"):
        assert callable(getattr(mg.ValueIteration, m))


def test_advantage_is_q_minus_v_on_valid_states():
    Q = np.array([[[0.5, 0.25], [0.0, 0.0]]], np.float32)
    r = mg.ActionValues(Q, np.array([[1, 0]], np.uint8), np.array([[0.5, 0.75]], np.float32), np.array([[0, -1]], np.int8),
                        3, "xyd")
    adv = r.advantage()
    assert adv.dtype == np.float32
    np.testing.assert_array_equal(adv, np.array([[[0.0, -0.25], [0.0, 0.0]]], np.float32))
    assert not np.signbit(adv[0, 1]).any()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ENVS))
def test_pi_star_is_the_lowest_optimal_action(name, dtype):
    model = ENVS[name][1]
    cells = cells_of(name)
    o = oracle.value_iteration(model, cells, gamma=0.99, tol=1e-6, dtype=dtype)
    assert o["dv"] == 0.0
    ref = qv.make_ref(model, cells, dtype=dtype)
    Q, opt = qv.q_and_opt(ref, o["V"])
    valid = ~ref.absorb
    assert valid.any()
    np.testing.assert_array_equal(Q.max(-1)[valid], o["V"][valid])
    np.testing.assert_array_equal(qv.lowest_bit(opt)[valid], o["pi"][valid])
    assert (opt[ref.absorb] == 0).all() and (Q[ref.absorb] == 0).all()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("slip,lava", [(None, "terminal"), (0.9, "terminal"), (None, "nodeath"), (0.9, "nodeath")])
def test_xyd_lanes_3_to_6_hold_the_same_bits(slip, lava, dtype):
    cells = cells_of("lava9")
    V = oracle.value_iteration_ex(0, cells, slip_p=slip, dtype=dtype, lava_mode=int(lava == "nodeath"))["V"]
    Q, opt = qv.q_and_opt(qv.make_ref(0, cells, slip_p=slip, dtype=dtype, lava=lava), V)
    raw = Q.view(np.uint32 if dtype == "f32" else np.uint64)
    for a in (4, 5, 6):
        np.testing.assert_array_equal(raw[..., a], raw[..., 3])
    hi = opt >> 3
    assert np.isin(hi, (0, 15)).all()


def test_nodeath_gives_a_negative_entry():
    cells = cells_of("lava9")
    ref = qv.make_ref(0, cells, dtype="f64", lava="nodeath", death_cost=-1.0)
    r = ref.policy_iteration(np.full((3, ref.S), 2, np.int8))
    Q, _ = qv.q_and_opt(ref, r["V"])
    assert Q.min() < 0


@pytest.mark.parametrize("name", ["empty5_a3", "empty5_a7", "empty6_a3"])
def test_learned_table_ties_with_q_star_per_state_and_action(name):
    """eps = 1, alpha = 1, unit_goal: every update is the oracle's backup, so the learner's table meets Q* of the
    restatement on the oracle's V* lane by lane (the first n_act lanes of every state with V* > 0), within
    section 18's tolerance."""
    c = qr.tie_case(name)
    cells = rr.cells_of(c["enc"])
    ref = qv.make_ref(0, cells, gamma=qr.TIE_GAMMA, tol=1e-13, dtype="f64")
    Q, _ = qv.q_and_opt(ref, c["V"])
    n = c["n_act"]
    on = c["V"] > 0
    assert on.any()
    err = np.abs(c["ref"]["Q"][..., :n] - Q[..., :n])[on].max()
    assert err <= qr.TIE_TOL, err


@pytest.mark.parametrize("name,slip", [("fourrooms", None), ("fourrooms", 0.9), ("doorkey5", None)])
def test_improve_changes_exactly_the_states_whose_lane_is_not_optimal(name, slip):
    model = ENVS[name][1]
    cells = cells_of(name)
    ref = qv.make_ref(model, cells, slip_p=slip, dtype="f32")
    rng = np.random.default_rng(7)
    valid = ~ref.absorb
    for pi in (rng.integers(0, ref.A, (ref.B, ref.S)).astype(np.int8), np.full((ref.B, ref.S), 2, np.int8)):
        V = ref.evaluate(pi)["V"]
        _, opt = qv.q_and_opt(ref, V)
        new, changed = ref.improve(V, pi)
        assert changed == int((valid & ~qv.lane_bit(opt, pi)).sum())
        assert changed > 0
        assert qv.lane_bit(opt, new)[valid].all()
