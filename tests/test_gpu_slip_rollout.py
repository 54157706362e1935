"""Slip rollouts on resident envs (csrc/envs_rollout.h SLIP = true) against the host
restatement tests/slip_ref.py: steps, fp64 return, flags, status, trace, the env state the call leaves and
every env's PCG64 record against numpy's own state integers, all array-equal.  Each _case_* function builds
its inputs and the restatement's result on the host and asserts there what the case is meant to contain."""
import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from oracle import oracle
from tests import rollout_ref as rr
from tests import slip_ref as sr

pytestmark = pytest.mark.gpu

STATE_KEYS = ("enc", "agent", "carry", "step_count")


def make_venv(env_id, enc, agent, **kw):
    venv = mg.MiniGridVecEnv(env_id, enc.shape[0], **kw)
    venv.load(enc, agent)
    return venv


def check_streams(got, streams):
    want = sr.stream_fields(streams) if isinstance(streams, list) else streams
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def check(res, st, streams, ref, trace=False):
    """Every output of a slip rollout, the env state and the streams it left, against the restatement's."""
    np.testing.assert_array_equal(res.status, ref["status"])
    np.testing.assert_array_equal(res.steps, ref["steps"])
    np.testing.assert_array_equal(res.ret, ref["ret"])
    np.testing.assert_array_equal(res.terminated, ref["terminated"])
    np.testing.assert_array_equal(res.truncated, ref["truncated"])
    for k in STATE_KEYS:
        np.testing.assert_array_equal(st[k], ref[k], err_msg=k)
    if trace:
        states, actions = rr.trim(ref)
        np.testing.assert_array_equal(res.states, states)
        np.testing.assert_array_equal(res.actions, actions)
    check_streams(streams, ref["streams"])


def ref_of(c, prob, seed0, sel=None, pi=None, **kw):
    sel = slice(None) if sel is None else sel
    pi = c["pi"][sel] if pi is None else pi
    return sr.slip_rollout_ref(c["enc"][sel], c["agent"][sel], pi, c["model"], c["max_steps"], prob, seed0,
                               see_through=c["see_through"], trace_len=c["max_steps"], **kw)


def run(c, prob, seed0, sel=None, pi=None, random_action=None, trace=True, **kw):
    sel = slice(None) if sel is None else sel
    venv = make_venv(c["env_id"], c["enc"][sel], c["agent"][sel])
    venv.set_slip(prob, seed=seed0, random_action=random_action)
    res = venv.rollout(c["pi"][sel] if pi is None else pi, model=c["model"], trace=trace, **kw)
    st, streams = venv.get_state(), venv.slip_streams()
    venv.close()
    return res, st, streams


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_small_batches(B):
    """A lone lane, a partial wave, exactly one wave, one env in a second wave."""
    c = rr.case("lava9n2")
    sel = np.arange(B)
    ref = ref_of(c, 0.7, 11, sel)
    assert ref["slipped"].any()
    res, st, streams = run(c, 0.7, 11, sel)
    check(res, st, streams, ref, trace=True)


# ---------------------------------------------------------------------------------------------- 2
def _case_doorkey(name, seed0=0):
    c = rr.case(name)
    ref = ref_of(c, 0.6, seed0)
    ev = ref["events"]
    assert any(e["action"] == sr.DROP and e["had_key"] and e["changed"] for e in ev), "no slipped drop of the key"
    assert any(e["action"] in (sr.PICKUP, sr.TOGGLE) and e["changed"] for e in ev), "no slipped pickup / toggle"
    return c, ref, seed0


@pytest.mark.parametrize("name", ["doorkey5", "doorkey8"])
def test_doorkey_mutations_through_slipped_actions(name):
    """A slipped drop leaves the DP's product state (the key lies elsewhere); the env executes it all the same."""
    c, ref, seed0 = _case_doorkey(name)
    res, st, streams = run(c, 0.6, seed0)
    check(res, st, streams, ref, trace=True)


# ---------------------------------------------------------------------------------------------- 3
def _case_continuation(seed0=0, first_n=4):
    c = rr.case("lava9n2")
    kw = dict(see_through=c["see_through"])
    one = ref_of(c, 0.7, seed0)
    ref1 = sr.slip_rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], 0.7, seed0, n_max=first_n,
                               trace_len=first_n, **kw)
    half = [b for b in range(65) if sum(n < first_n for n in one["int_draw_steps"][b]) % 2 == 1
            and any(n >= first_n for n in one["int_draw_steps"][b])]
    assert half, "no env enters the second call with a buffered half-word it goes on to use"
    assert all(ref1["streams"][b]["has_uint32"] == 1 for b in half)
    ref2 = sr.continue_ref(ref1, c["pi"], c["model"], c["max_steps"], 0.7, trace_len=c["max_steps"], **kw)
    return c, one, ref1, ref2, seed0, first_n


def test_continuation_keeps_the_half_word_buffer():
    """integers(0, 6) consumes one 32-bit half of a draw and buffers the other: a call that ends after an odd
    number of them hands has_uint32 / uinteger to the next one."""
    c, one, ref1, ref2, seed0, first_n = _case_continuation()
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    venv.set_slip(0.7, seed=seed0)
    r1 = venv.rollout(c["pi"], max_steps=first_n, trace=True)
    check(r1, venv.get_state(), venv.slip_streams(), ref1, trace=True)
    r2 = venv.rollout(c["pi"], trace=True)
    st, streams = venv.get_state(), venv.slip_streams()
    venv.close()
    check(r2, st, streams, ref2, trace=True)
    np.testing.assert_array_equal(r1.steps + r2.steps, one["steps"])
    for k in STATE_KEYS:
        np.testing.assert_array_equal(st[k], one[k], err_msg=k)
    check_streams(streams, one["streams"])


# ---------------------------------------------------------------------------------------------- 4
def test_prob_one_is_the_plain_rollout():
    c = rr.case("lava9n2")
    plain = c["ref"]
    res, st, streams = run(c, 1.0, 5)
    np.testing.assert_array_equal(res.steps, plain["steps"])
    np.testing.assert_array_equal(res.ret, plain["ret"])
    np.testing.assert_array_equal(res.status, plain["status"])
    np.testing.assert_array_equal(res.terminated, plain["terminated"])
    np.testing.assert_array_equal(res.truncated, plain["truncated"])
    states, actions = rr.trim(plain)
    np.testing.assert_array_equal(res.states, states)
    np.testing.assert_array_equal(res.actions, actions)
    for k in STATE_KEYS:
        np.testing.assert_array_equal(st[k], plain[k], err_msg=k)
    check_streams(streams, sr.fresh_streams(5, 65, doubles=plain["steps"]))  # one random() per step taken


def test_prob_zero_draws_every_action():
    c = rr.case("lava9n2")
    ref = ref_of(c, 0.0, 2)
    taken = np.arange(c["max_steps"])[:, None] < ref["steps"][None, :]
    np.testing.assert_array_equal(ref["slipped"], taken)
    assert all(len(ref["int_draw_steps"][b]) == ref["steps"][b] for b in range(65))
    assert ref["actions"].max() == 5  # 0..5: done (6) is never drawn
    res, st, streams = run(c, 0.0, 2)
    check(res, st, streams, ref, trace=True)


def test_a_fixed_random_action_draws_doubles_only():
    c = rr.case("lava9n2")
    ref = ref_of(c, 0.5, 3, random_action=2)
    assert ref["slipped"].any() and (ref["actions"][ref["slipped"]] == 2).all()
    res, st, streams = run(c, 0.5, 3, random_action=2)
    check(res, st, streams, ref, trace=True)
    check_streams(streams, sr.fresh_streams(3, 65, doubles=ref["steps"]))


# ---------------------------------------------------------------------------------------------- 5
def test_seeding():
    c = rr.case("lava9n2")
    # SeedSequence takes 2^32 - 1 as one 32-bit word and 2^32, 2^32 + 1 as two
    seed0 = 2**32 - 1
    sel = np.arange(3)
    venv = make_venv(c["env_id"], c["enc"][sel], c["agent"][sel])
    venv.set_slip(0.7, seed=seed0)
    check_streams(venv.slip_streams(), sr.fresh_streams(seed0, 3))
    # a masked reseed changes only the masked envs; load() and get_state() touch no stream
    venv.set_slip(0.7, seed=100, mask=np.array([1, 0, 1], np.uint8))
    venv.load(c["enc"][sel], c["agent"][sel])
    a, b = sr.fresh_streams(100, 3), sr.fresh_streams(seed0, 3)
    want = {k: np.where(np.array([True, False, True]), a[k], b[k]) for k in a}
    check_streams(venv.slip_streams(), want)
    venv.close()
    # the same seed twice reproduces a rollout
    first = run(c, 0.7, 21)
    second = run(c, 0.7, 21)
    check(second[0], second[1], second[2], ref_of(c, 0.7, 21), trace=True)
    np.testing.assert_array_equal(first[0].ret, second[0].ret)
    np.testing.assert_array_equal(first[0].actions, second[0].actions)
    check_streams(first[2], second[2])
    # env b of the batch == that env alone with seed0 + b: lane 0 of its own wave instead of lane b / wave 1
    for b in (0, 37, 64):
        res, st, streams = run(c, 0.7, 21 + b, sel=np.array([b]))
        assert res.steps[0] == first[0].steps[b] and res.ret[0] == first[0].ret[b]
        k = int(res.steps[0])
        np.testing.assert_array_equal(res.actions[:k, 0], first[0].actions[:k, b])
        for key in STATE_KEYS:
            np.testing.assert_array_equal(st[key][0], first[1][key][b], err_msg=key)
        for key in streams:
            assert streams[key][0] == first[2][key][b], key


# ---------------------------------------------------------------------------------------------- 6
def _case_step_loop(name, seed0, n=10):
    c = rr.case(name)
    ref = sr.slip_rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], 0.7, seed0,
                              see_through=c["see_through"], n_max=n, trace_len=n)
    full = (ref["steps"] == n) & ~ref["terminated"] & ~ref["truncated"]
    assert full.sum() > 32 and ref["slipped"].any()
    return c, ref, full, seed0, n


@pytest.mark.parametrize("name,seed0", [("lava9n2", 0), ("doorkey8", 0)])
def test_slip_actions_against_the_fused_loop(name, seed0):
    """policy_actions_device -> slip_actions_device -> step_device for 10 steps == rollout(max_steps=10) ==
    the restatement.  An env that ends earlier gets -1 from the lookup, which slip_actions passes through
    without a draw and step() refuses (counting the step), so states are compared on the envs that run all 10
    steps and streams on every env."""
    import torch

    c, ref, full, seed0, n = _case_step_loop(name, seed0)
    model, pi, B = c["model"], c["pi"], 65
    a = make_venv(c["env_id"], c["enc"], c["agent"])
    b = make_venv(c["env_id"], c["enc"], c["agent"])
    a.set_slip(0.7, seed=seed0)
    b.set_slip(0.7, seed=seed0)
    dev = torch.device("cuda", 0)
    pi_d = torch.from_numpy(np.ascontiguousarray(pi)).to(dev)
    act_d = torch.zeros(B, dtype=torch.int32, device=dev)
    out_d = torch.zeros((n, B), dtype=torch.int32, device=dev)  # row k: the actions executed at step k
    stat_d = torch.zeros(B, dtype=torch.int32, device=dev)
    obs = torch.zeros((B, a.view, a.view, 3), dtype=torch.uint8, device=dev)
    direction = torch.zeros(B, dtype=torch.int32, device=dev)
    rew = torch.zeros(B, dtype=torch.float64, device=dev)
    term = torch.zeros(B, dtype=torch.uint8, device=dev)
    trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
    sstat = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for k in range(n):  # one stream: each launch sees the one before it
        a.policy_actions_device(pi_d, 1, model, act_d, stat_d)
        a.slip_actions_device(act_d, out_d[k])
        a.step_device(out_d[k], obs, direction, rew, term, trunc, sstat)
    sa, streams_a = a.get_state(), a.slip_streams()
    acts = out_d.cpu().numpy()
    res = b.rollout(pi, model=model, max_steps=n, trace=True)
    sb, streams_b = b.get_state(), b.slip_streams()
    # the host entry point, in place of the device one, for one more decision on a's streams
    extra = a.slip_actions(np.where(full, 2, -1))
    a.close()
    b.close()
    check(res, sb, streams_b, ref, trace=True)
    for k in STATE_KEYS:
        np.testing.assert_array_equal(sa[k][full], sb[k][full], err_msg=k)
    np.testing.assert_array_equal(acts[:, full], res.actions[:, full])
    np.testing.assert_array_equal(acts[:, full], ref["actions"][:n][:, full])
    check_streams(streams_a, streams_b)
    want = [sr.slip_decide(r, 0.7, None, 2)[0] if f else -1 for r, f in zip(ref["rngs"], full)]
    np.testing.assert_array_equal(extra, want)


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("W,reader,seed", [(51, "hbm", 5), (19, "lds", 3)])
def test_both_cell_readers(W, reader, seed):
    """The random walled grids of test_gpu_policy_rollout.test_both_cell_readers under slip: 51 x 51 steps on
    the env's plane in HBM, 19 x 19 on LDS."""
    from tests.test_gpu_policy_rollout import _random_case

    assert (64 * ((W * W + 15) // 16 * 16 + 4) > 160 * 1024) == (reader == "hbm")
    enc, agent, pi = _random_case(W, seed=seed)
    ms = 4 * W * W
    ref = sr.slip_rollout_ref(enc, agent, pi, "xyd", ms, 0.9, 4, see_through=True, n_max=300, trace_len=300)
    assert ref["slipped"].any() and (ref["steps"] > 20).any()
    venv = mg.MiniGridVecEnv("MiniGrid-Empty-5x5-v0", 3, size=W)
    venv.load(enc, agent)
    venv.set_slip(0.9, seed=4)
    res = venv.rollout(pi, model="xyd", max_steps=300, trace=True)
    st, streams = venv.get_state(), venv.slip_streams()
    venv.close()
    check(res, st, streams, ref, trace=True)


@pytest.mark.parametrize("knob", [{"MGDP_ROLLOUT_READER": "hbm"}])
def test_the_ab_sides_compute_the_same(knob, monkeypatch):
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    c = rr.case("lava9n2")
    res, st, streams = run(c, 0.7, 11)
    check(res, st, streams, ref_of(c, 0.7, 11), trace=True)


# ---------------------------------------------------------------------------------------------- 8
def _case_time_indexed():
    c = rr.case("lava9n2")
    pit = rr.noisy_policy(c["pi"], "xyd", 0.3, seed0=50, T=c["max_steps"])
    ref = ref_of(c, 0.7, 9, pi=pit)
    assert ref["slipped"].any() and (ref["steps"] > 100).any()  # some env walks through a hundred rows
    return c, pit, ref


def test_time_indexed_policy_under_slip():
    c, pit, ref = _case_time_indexed()
    res, st, streams = run(c, 0.7, 9, pi=pit)
    check(res, st, streams, ref, trace=True)


def _case_nodeath():
    env_id, B, dc = "MiniGrid-LavaCrossingS9N1-v0", 64, -0.75
    enc, agent, env = rr.grids(env_id, B)
    pi = oracle.value_iteration_ex(0, rr.cells_of(enc), dtype="f64", lava_mode=1, death_cost=dc)["pi"]
    ms = env.max_steps
    ref = sr.slip_rollout_ref(enc, agent, pi, "xyd", ms, 0.2, 0, see_through=env.see_through_walls, trace_len=ms,
                              nd_types=("lava",), death_cost=dc)
    # the goal reward is >= 0, so a return below one cost holds at least two of them; pi* itself never pays
    assert (ref["ret"] < dc).any(), "the case needs an env that paid the death cost twice"
    return env_id, enc, agent, pi, dc, ref


def test_nodeath_costs_accumulate_in_step_order_on_the_executed_action():
    env_id, enc, agent, pi, dc, ref = _case_nodeath()
    venv = make_venv(env_id, enc, agent, no_death_types=("lava",), death_cost=dc)
    venv.set_slip(0.2, seed=0)
    res = venv.rollout(pi, trace=True)
    st, streams = venv.get_state(), venv.slip_streams()
    venv.close()
    check(res, st, streams, ref, trace=True)


# ---------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("env_id", ["MiniGrid-Empty-8x8-v0", "MiniGrid-LavaCrossingS9N1-v0"])
def test_the_dp_slip_model_against_the_env(env_id):
    """pi* and V* of the slip_p = 0.8 DP (gamma 0.9, fp64), 4096 copies of the reset(seed=0) grid rolled out
    under set_slip(0.8, seed=0): |mean(g) - V*[start]| <= 4 std(g, ddof=1) / sqrt(B), g = gamma^(steps-1) on
    the goal and 0 elsewhere.  The restatement alone gives z = -0.89 (Empty-8x8) and +0.87 (LavaCrossingS9N1)."""
    c = sr.stat_case(env_id)
    ref, B = c["ref"], c["enc"].shape[0]
    venv = mg.MiniGridVecEnv(env_id, B)
    venv.load(c["enc"], c["agent"], max_steps=c["max_steps"])
    venv.set_slip(c["prob"], seed=c["seed0"])
    res = venv.rollout(c["pi"], model="xyd")
    streams = venv.slip_streams()
    venv.close()
    g = sr.discounted_goal(res.steps, res.ret, res.terminated, c["gamma"])
    mean, z = sr.z_score(g, c["v_start"])
    print(f"{env_id}: V*[start] = {c['v_start']:.6f}, mean = {mean:.6f}, z = {z:+.2f}")
    np.testing.assert_array_equal(res.steps, ref["steps"])
    np.testing.assert_array_equal(res.terminated, ref["terminated"])
    np.testing.assert_array_equal(res.truncated, ref["truncated"])
    np.testing.assert_array_equal(res.ret, ref["ret"])
    check_streams(streams, ref["streams"])
    assert abs(z) <= 4.0


# ---------------------------------------------------------------------------------------------- 10
def test_call_level_errors_raise_value_error():
    c = rr.case("lava9n2")
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    acts = np.zeros(65, np.int32)
    with pytest.raises(ValueError):
        venv.slip_actions(acts)  # before set_slip
    with pytest.raises(ValueError):
        venv.slip_streams()
    with pytest.raises(ValueError):
        venv.set_slip(0.7, mask=np.ones(65, np.uint8))  # a masked first call
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            venv.set_slip(bad)
    for bad in (7, -1, -2):
        with pytest.raises(ValueError):
            venv.set_slip(0.7, random_action=bad)
    with pytest.raises(ValueError):
        venv.set_slip(0.7, seed=-1)
    with pytest.raises(ValueError):
        venv.slip_actions(acts)  # no refused call set anything
    venv.set_slip(0.7, random_action=6)  # done: an env action, though never drawn
    venv.set_slip(0.7, seed=1, mask=np.ones(65, np.uint8))
    venv.clear_slip()
    with pytest.raises(ValueError):
        venv.slip_actions(acts)
    with pytest.raises(ValueError):
        venv.set_slip(0.7, mask=np.ones(65, np.uint8))  # a first call again
    res = venv.rollout(c["pi"])  # and the plain rollout again
    np.testing.assert_array_equal(res.steps, c["ref"]["steps"])
    np.testing.assert_array_equal(res.ret, c["ref"]["ret"])
    venv.close()
    venv = mg.MiniGridVecEnv(c["env_id"], 65, autoreset=True)
    venv.load(c["enc"], c["agent"])
    venv.set_slip(0.7)
    with pytest.raises(ValueError):
        venv.rollout(c["pi"])  # as without slip
    venv.close()
