"""The slip rollout's host restatement (tests/slip_ref.py) on its own: without noise it is
the section 16 restatement, and the DP's slip model predicts what it collects."""
import numpy as np
import pytest

from tests import rollout_ref as rr
from tests import slip_ref as sr


@pytest.mark.parametrize("name", ["lava9n2", "doorkey5"])
def test_prob_one_is_the_plain_restatement(name):
    c = rr.case(name)
    ms = c["max_steps"]
    r = sr.slip_rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], ms, 1.0, seed0=7, see_through=c["see_through"],
                            trace_len=ms)
    for k in ("steps", "ret", "terminated", "truncated", "status", "states", "actions", "enc", "agent", "carry",
              "step_count"):
        np.testing.assert_array_equal(r[k], c["ref"][k], err_msg=k)
    assert not r["slipped"].any() and not r["events"] and not any(r["int_draw_steps"])
    # one random() per step taken and nothing else
    want = sr.fresh_streams(7, len(r["steps"]), doubles=r["steps"])
    got = sr.stream_fields(r["streams"])
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_a_fixed_random_action_draws_doubles_only():
    c = rr.case("lava9n2")
    r = sr.slip_rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], 0.5, seed0=3, random_action=2,
                            see_through=c["see_through"], trace_len=c["max_steps"])
    assert r["slipped"].any() and (r["actions"][r["slipped"]] == 2).all()
    want = sr.fresh_streams(3, 65, doubles=r["steps"])
    got = sr.stream_fields(r["streams"])
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_budgeted_then_unbudgeted_equals_one_call():
    c = rr.case("lava9n2")
    kw = dict(see_through=c["see_through"])
    one = sr.slip_rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], 0.7, seed0=0, **kw)
    first = sr.slip_rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], 0.7, seed0=0, n_max=4, **kw)
    second = sr.continue_ref(first, c["pi"], c["model"], c["max_steps"], 0.7, **kw)
    np.testing.assert_array_equal(first["steps"] + second["steps"], one["steps"])
    for k in ("enc", "agent", "carry", "step_count"):
        np.testing.assert_array_equal(second[k], one[k], err_msg=k)
    assert second["streams"] == one["streams"]


@pytest.mark.parametrize("env_id", ["MiniGrid-Empty-8x8-v0", "MiniGrid-LavaCrossingS9N1-v0"])
def test_the_dp_slip_model_predicts_the_restatement(env_id):
    """4096 rollouts of pi* (slip_p = 0.8, gamma = 0.9) under set_slip(0.8, seed=0): the mean discounted
    goal indicator lies within 4 standard errors of V*[start]."""
    c = sr.stat_case(env_id)
    r = c["ref"]
    assert (r["status"] == 0).all() and not r["truncated"].any()
    g = sr.discounted_goal(r["steps"], r["ret"], r["terminated"], c["gamma"])
    mean, z = sr.z_score(g, c["v_start"])
    print(f"{env_id}: V*[start] = {c['v_start']:.6f}, mean = {mean:.6f}, z = {z:+.2f}")
    assert abs(z) <= 4.0
