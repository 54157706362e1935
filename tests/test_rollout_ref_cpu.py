"""The host restatement of the policy rollout (tests/rollout_ref.py) and the inputs the GPU tests of
tests/test_gpu_policy_rollout.py rely on, pinned without a GPU: pi* collects V*[start], the noisy-policy
cases contain every ending, every mutation and a bad lane, and a budgeted call continues exactly."""
import numpy as np
import pytest

from tests import rollout_ref as rr

GAMMA = 0.99
KEY = rr.KEY


@pytest.mark.parametrize("env_id,model", [("MiniGrid-Empty-5x5-v0", "xyd"), ("MiniGrid-DoorKey-5x5-v0", "doorkey")])
def test_optimal_policy_reaches_the_goal_with_v_start(env_id, model):
    B = 16
    enc, agent, env = rr.grids(env_id, B)
    V, pi = rr.oracle_policy(enc, model, gamma=GAMMA)
    r = rr.rollout_ref(enc, agent, pi, model, env.max_steps, env.see_through_walls)
    v0 = V[np.arange(B), rr.start_states(enc, agent, model)]
    assert (v0 > 0).all(), "every seed of these families is solvable"
    assert (r["status"] == 0).all() and r["terminated"].all() and not r["truncated"].any()
    for b in range(B):
        n = int(r["steps"][b])
        assert v0[b] == rr.gamma_pow(GAMMA, n), (b, n, v0[b])
        assert r["ret"][b] == 1.0 - 0.9 * (n / env.max_steps)  # _reward, minigrid_env.py:240
        assert r["step_count"][b] == n


def _endings(ref):
    goal = ref["terminated"] & (ref["ret"] > 0)
    lava = ref["terminated"] & (ref["ret"] == 0)
    return int(goal.sum()), int(lava.sum()), int(ref["truncated"].sum())


def _door_open(ref, b):
    t = ref["enc"][b]
    door = t[t[..., 0] == rr.DOOR]
    return len(door) == 1 and door[0][2] == 0


def test_noisy_lava_case_contains_every_ending():
    c = rr.case("lava9n2")
    ref = c["ref"]
    goal, lava, trunc = _endings(ref)
    assert goal >= 1 and lava >= 1 and trunc >= 1 and goal + lava + trunc == 65
    assert (ref["status"] == 0).all()
    assert (ref["steps"][ref["truncated"]] == c["max_steps"]).all()
    # the trace holds exactly the steps taken
    for b in range(65):
        n = int(ref["steps"][b])
        assert (ref["states"][:n, b] >= 0).all() and (ref["states"][n:, b] == -1).all()
        assert (ref["actions"][:n, b] >= 0).all() and (ref["actions"][n:, b] == -1).all()
    # a budget of 12 leaves envs running, and finished ones too
    b12 = rr.rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], c["see_through"], n_max=12)
    running = (b12["steps"] == 12) & ~b12["terminated"] & ~b12["truncated"]
    assert running.any() and not running.all()


def test_budgeted_then_unbudgeted_equals_one_call():
    c = rr.case("lava9n2")
    kw = dict(see_through=c["see_through"])
    first = rr.rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], n_max=12, **kw)
    second = rr.continue_ref(first, c["pi"], c["model"], c["max_steps"], **kw)
    ref = c["ref"]
    np.testing.assert_array_equal(first["steps"] + second["steps"], ref["steps"])
    for k in ("enc", "agent", "carry", "step_count"):
        np.testing.assert_array_equal(second[k], ref[k])
    # an env that ended inside the budget stands on an absorbing state: its lane is -1
    ended = first["terminated"]
    assert ended.any() and (second["status"][ended] == rr.E_ACTION).all() and (second["steps"][ended] == 0).all()


@pytest.mark.parametrize("name", ["doorkey5", "doorkey8"])
def test_noisy_doorkey_cases_pick_up_and_open(name):
    c = rr.case(name)
    ref = c["ref"]
    goal, lava, trunc = _endings(ref)
    assert goal >= 1 and trunc >= 1 and lava == 0
    picked = ref["carry"][:, 0] == KEY
    assert picked.any() and not picked.all()
    for b in np.flatnonzero(picked):  # the key left its cell
        assert not (ref["enc"][b][..., 0] == KEY).any()
    opened = np.array([_door_open(ref, b) for b in range(65)])
    assert opened.any() and not opened.all()
    # has_key and door_open both show in the visited state indices (the two low bits)
    s = ref["states"][ref["states"] >= 0]
    assert ((s & 3) == 0).any() and ((s & 3) == 2).any() and ((s & 3) == 3).any()


def test_bad_policy_case_stops_on_its_lane():
    c = rr.case("lava9n2")
    pi, states = rr.bad_policy(c)
    r = rr.rollout_ref(c["enc"], c["agent"], pi, c["model"], c["max_steps"], c["see_through"])
    ref = c["ref"]
    for b, lane in ((3, -1), (7, 7)):
        first = int(np.flatnonzero(ref["states"][:, b] == states[b])[0])
        assert r["status"][b] == rr.E_ACTION and r["steps"][b] == first
        assert not r["terminated"][b] and not r["truncated"][b]
    others = np.ones(65, bool)
    others[[3, 7]] = False
    for k in ("steps", "ret", "status", "terminated", "truncated"):
        np.testing.assert_array_equal(r[k][others], ref[k][others])


def test_model_status_refuses_what_is_outside_the_model():
    c = rr.case("lava9n2")
    enc = c["enc"][0].copy()
    assert rr.model_status("xyd", enc, (0, 0)) == 0
    assert rr.model_status("xyd", enc, (6, 1)) == rr.E_UNSUPPORTED  # a carried ball
    enc[2, 2] = (6, 1, 0)  # a ball on the grid
    assert rr.model_status("xyd", enc, (0, 0)) == rr.E_UNSUPPORTED
    d = rr.case("doorkey5")
    enc = d["enc"][0]
    assert rr.model_status("doorkey", enc, (0, 0)) == 0
    assert rr.model_status("doorkey", enc, (KEY, 4)) == rr.E_UNSUPPORTED  # a second key of the colour
    assert rr.model_status("xyd", enc, (0, 0)) == rr.E_UNSUPPORTED
    fin = d["ref"]
    b = int(np.flatnonzero(fin["carry"][:, 0] == KEY)[0])
    assert rr.model_status("doorkey", fin["enc"][b], fin["carry"][b]) == 0  # the key in hand
    assert rr.model_status("doorkey", fin["enc"][b], (0, 0)) == rr.E_UNSUPPORTED  # no key anywhere
