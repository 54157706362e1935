"""Tabular policies executed on resident envs (csrc/envs_rollout.h): the fused
rollout and the policy lookup against the host restatement tests/rollout_ref.py, bit for bit on every
output -- steps, fp64 return, flags, status, trace and the env state the call leaves behind."""
import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from minigrid_dynamicprogramming_amd import _lib
from minigrid_dynamicprogramming_amd.dp import DOORKEY_ACTIONS, state_index
from tests import rollout_ref as rr
from tests.test_gpu_wave2 import random_grids

pytestmark = pytest.mark.gpu


def make_venv(env_id, enc, agent, **kw):
    venv = mg.MiniGridVecEnv(env_id, enc.shape[0], **kw)
    venv.load(enc, agent)
    return venv


def check(res, st, ref, trace=False):
    """Every output of a rollout and the state it left, against the reference's."""
    np.testing.assert_array_equal(res.status, ref["status"])
    np.testing.assert_array_equal(res.steps, ref["steps"])
    np.testing.assert_array_equal(res.ret, ref["ret"])
    np.testing.assert_array_equal(res.terminated, ref["terminated"])
    np.testing.assert_array_equal(res.truncated, ref["truncated"])
    for k in ("enc", "agent", "carry", "step_count"):
        np.testing.assert_array_equal(st[k], ref[k], err_msg=k)
    if trace:
        states, actions = rr.trim(ref)
        np.testing.assert_array_equal(res.states, states)
        np.testing.assert_array_equal(res.actions, actions)
    else:
        assert res.states is None and res.actions is None
    assert res.ok == bool((ref["status"] == 0).all())


def run_case(c, sel=None, trace=False, **kw):
    sel = slice(None) if sel is None else sel
    venv = make_venv(c["env_id"], c["enc"][sel], c["agent"][sel])
    res = venv.rollout(c["pi"][sel], model=c["model"], trace=trace, **kw)
    st = venv.get_state()
    venv.close()
    return res, st


@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_small_batches(B):
    """A lone lane, a partial wave, exactly one wave, one env in a second wave."""
    env_id = "MiniGrid-Empty-5x5-v0"
    enc, agent, env = rr.grids(env_id, B)
    V, pi = rr.oracle_policy(enc, "xyd")
    ref = rr.rollout_ref(enc, agent, pi, "xyd", env.max_steps, env.see_through_walls)
    venv = make_venv(env_id, enc, agent)
    res = venv.rollout(pi)  # model="auto"
    check(res, venv.get_state(), ref)
    venv.close()
    assert res.terminated.all() and (res.ret > 0).all()
    v0 = V[np.arange(B), rr.start_states(enc, agent, "xyd")]
    assert all(v0[b] == rr.gamma_pow(0.99, int(res.steps[b])) for b in range(B))


def test_every_ending_in_one_wave_with_trace():
    c = rr.case("lava9n2")
    res, st = run_case(c, trace=True)
    check(res, st, c["ref"], trace=True)
    goal = res.terminated & (res.ret > 0)
    lava = res.terminated & (res.ret == 0)
    assert goal.any() and lava.any() and res.truncated.any()
    head, _ = run_case(c, trace=5)  # the first five steps only
    np.testing.assert_array_equal(head.states, c["ref"]["states"][:5])
    np.testing.assert_array_equal(head.actions, c["ref"]["actions"][:5])
    np.testing.assert_array_equal(head.steps, res.steps)


def test_budget_then_unbudgeted_call():
    c = rr.case("lava9n2")
    kw = dict(see_through=c["see_through"])
    ref1 = rr.rollout_ref(c["enc"], c["agent"], c["pi"], c["model"], c["max_steps"], n_max=12, **kw)
    ref2 = rr.continue_ref(ref1, c["pi"], c["model"], c["max_steps"], **kw)
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    r1 = venv.rollout(c["pi"], max_steps=12)
    check(r1, venv.get_state(), ref1)
    r2 = venv.rollout(c["pi"])
    st = venv.get_state()
    check(r2, st, ref2)
    venv.close()
    # ... and one unbudgeted call: the same final state, the same steps in sum
    one = c["ref"]
    np.testing.assert_array_equal(r1.steps + r2.steps, one["steps"])
    for k in ("enc", "agent", "carry", "step_count"):
        np.testing.assert_array_equal(st[k], one[k])
    running = (r1.steps == 12) & ~r1.terminated & ~r1.truncated
    assert running.any() and not running.all()


@pytest.mark.parametrize("name", ["doorkey5", "doorkey8"])
def test_mutations(name):
    """pickup empties the key's cell and fills the carry, toggle changes the door's state."""
    c = rr.case(name)
    res, st = run_case(c, trace=True)
    check(res, st, c["ref"], trace=True)
    picked = st["carry"][:, 0] == rr.KEY
    assert picked.any() and not picked.all()
    assert not (st["enc"][picked][..., 0] == rr.KEY).any()
    t = st["enc"]
    opened = np.array([(t[b][t[b][..., 0] == rr.DOOR][0][2] == 0) for b in range(t.shape[0])])
    assert opened.any() and not opened.all()


def test_envs_are_independent_of_their_wave_position():
    c = rr.case("lava9n2")
    sel = np.concatenate([np.arange(32), np.arange(32)])
    res, st = run_case(c, sel=sel, trace=True)
    for a in (res.steps, res.ret, res.terminated, res.truncated, res.status, st["enc"], st["agent"], st["step_count"]):
        np.testing.assert_array_equal(a[:32], a[32:])
    np.testing.assert_array_equal(res.states[:, :32], res.states[:, 32:])
    ref = c["ref"]
    np.testing.assert_array_equal(res.steps[:32], ref["steps"][:32])
    np.testing.assert_array_equal(res.ret[:32], ref["ret"][:32])
    # and of the batch around them: the same envs alone
    alone, _ = run_case(c, sel=np.arange(5))
    np.testing.assert_array_equal(alone.steps, ref["steps"][:5])
    np.testing.assert_array_equal(alone.ret, ref["ret"][:5])


@pytest.mark.parametrize("env_id", ["MiniGrid-DoorKey-5x5-v0", "MiniGrid-LavaGapS6-v0"])
def test_time_indexed_policy_collects_exactly_v0(env_id):
    B = 16
    model = "doorkey" if "DoorKey" in env_id else "xyd"
    enc, agent, env = rr.grids(env_id, B)
    Hh = env.max_steps
    vi = mg.ValueIteration(enc, model=model, gamma=1.0, dtype="f64", horizon=Hh, keep_policy_t=True)
    vi.solve()
    V0 = vi.values()
    pit = vi.policy_t()
    vi.close()
    ref = rr.rollout_ref(enc, agent, pit, model, Hh, env.see_through_walls)
    venv = make_venv(env_id, enc, agent)
    res = venv.rollout(pit, model=model)
    check(res, venv.get_state(), ref)
    v0 = V0[np.arange(B), rr.start_states(enc, agent, model)]
    np.testing.assert_array_equal(res.ret, v0)
    assert (v0 > 0).any() and res.ok
    # a policy shorter than the episode: MGDP_E_INVALID at step_count == T, the env as that many steps left it
    Ts = 3
    assert (res.steps > Ts).any()
    ref_s = rr.rollout_ref(enc, agent, pit[:Ts], model, Hh, env.see_through_walls)
    venv.load(enc, agent)
    short = venv.rollout(pit[:Ts], model=model)
    st = venv.get_state()
    venv.close()
    check(short, st, ref_s)
    cut = res.steps > Ts
    assert (short.status[cut] == _lib.MGDP_E_INVALID).all() and (short.steps[cut] == Ts).all()
    assert (st["step_count"][cut] == Ts).all()
    assert (short.status[~cut] == 0).all()


def test_nodeath_costs_accumulate_in_step_order():
    env_id, B, dc = "MiniGrid-LavaCrossingS9N1-v0", 64, -0.75
    enc, agent, env = rr.grids(env_id, B)
    vi = mg.ValueIteration(enc, model="xyd", dtype="f64", lava="nodeath", death_cost=dc)
    vi.solve()
    pi = vi.policy()
    vi.close()
    # time-indexed noise over (left, right, forward): the agent keeps wandering and walks into the lava
    pit = rr.noisy_policy(pi, "xyd", 0.5, lanes=3, T=env.max_steps)
    ref = rr.rollout_ref(enc, agent, pit, "xyd", env.max_steps, env.see_through_walls, nd_types=("lava",),
                         death_cost=dc, trace_len=env.max_steps)
    # the goal reward is >= 0, so a return below one cost holds at least two of them
    assert (ref["ret"] < dc).any(), "the case needs an env that paid the death cost twice"
    venv = make_venv(env_id, enc, agent, no_death_types=("lava",), death_cost=dc)
    res = venv.rollout(pit, trace=True)
    check(res, venv.get_state(), ref, trace=True)
    venv.close()


def _random_case(W, seed, B=3):
    """Random-obstacle XYD grids of one size; the agents start on solvable empty cells: the farthest from
    the goal, and the ones at 3/4 and 19/20 of the way up the order of V*.  Noise 0.02: over dozens of
    states to the goal a stationary policy with more of it only spins in place."""
    cells = random_grids(B, W, W, seed=seed)  # (B, H, W) type codes
    colour = np.zeros(16, np.uint8)
    colour[[2, 3, 8, 9]] = (5, 2, 1, 0)  # wall grey, floor blue, goal green, lava red (Grid.encode())
    enc = np.zeros((B, W, W, 3), np.uint8)
    enc[..., 0] = cells.transpose(0, 2, 1)
    enc[..., 1] = colour[enc[..., 0]]
    V, pi = rr.oracle_policy(enc, "xyd")
    agent = np.zeros((B, 3), np.int32)
    for b in range(B):
        v = V[b].reshape(W, W, 4)[:, :, 0]  # [y][x], heading east
        ys, xs = np.nonzero((cells[b] == 1) & (v > 0))
        assert len(ys), "no solvable start in this grid"
        k = np.argsort(v[ys, xs])[int((len(ys) - 1) * (0, 0.75, 0.95)[b % 3])]
        agent[b] = (xs[k], ys[k], 0)
    return enc, agent, rr.noisy_policy(pi, "xyd", 0.02)


@pytest.mark.parametrize("W,reader,seed", [(51, "hbm", 5), (19, "lds", 3)])
def test_both_cell_readers(W, reader, seed):
    """51 x 51: 64 padded planes exceed a CU's LDS, the loop reads the env's plane in HBM; 19 x 19: the
    same inputs' recipe through the LDS reader.  B = 3, budget 300."""
    assert (64 * ((W * W + 15) // 16 * 16 + 4) > 160 * 1024) == (reader == "hbm")
    enc, agent, pi = _random_case(W, seed=seed)
    ms = 4 * W * W
    ref = rr.rollout_ref(enc, agent, pi, "xyd", ms, True, n_max=300, trace_len=300)
    assert ref["terminated"].any() and ((ref["steps"] == 300) & ~ref["terminated"]).any()  # an ending and the budget
    venv = mg.MiniGridVecEnv("MiniGrid-Empty-5x5-v0", 3, size=W)
    assert (venv.W, venv.H, venv.max_steps, venv.see_through) == (W, W, ms, True)
    venv.load(enc, agent)
    res = venv.rollout(pi, model="xyd", max_steps=300, trace=True)
    check(res, venv.get_state(), ref, trace=True)
    venv.close()


def _expected_actions(st, pi, model, W):
    B = st["agent"].shape[0]
    out = np.full(B, -1, np.int32)
    for b in range(B):
        x, y, d = (int(v) for v in st["agent"][b])
        hk = dop = 0
        if model == "doorkey":
            hk = int(st["carry"][b, 0] == rr.KEY)
            t = st["enc"][b]
            dop = int(t[t[..., 0] == rr.DOOR][0][2] == 0)
        lane = int(pi[b, state_index(model, W, x, y, d, hk, dop)])
        if lane >= 0:
            out[b] = DOORKEY_ACTIONS[lane] if model == "doorkey" else lane
    return out


@pytest.mark.parametrize("name", ["lava9n2", "doorkey8"])
def test_policy_actions(name):
    import torch

    c = rr.case(name)
    model, pi = c["model"], c["pi"]
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    acts, status = venv.policy_actions(pi, model=model, return_status=True)
    np.testing.assert_array_equal(acts, _expected_actions(venv.get_state(), pi, model, venv.W))
    assert (acts >= 0).all() and (status == 0).all()
    venv.rollout(pi, model=model, max_steps=30)
    acts, status = venv.policy_actions(pi, model=model, return_status=True)
    np.testing.assert_array_equal(acts, _expected_actions(venv.get_state(), pi, model, venv.W))
    np.testing.assert_array_equal(status == 0, acts >= 0)  # an env that ended stands on an absorbing state
    venv.close()
    # its output fed to step_device for 20 steps == rollout(max_steps=20), on the envs that run that long
    sel = np.flatnonzero(c["ref"]["steps"] > 20)
    B = len(sel)
    assert B > 32
    a = make_venv(c["env_id"], c["enc"][sel], c["agent"][sel])
    b = make_venv(c["env_id"], c["enc"][sel], c["agent"][sel])
    dev = torch.device("cuda", 0)
    pi_d = torch.from_numpy(np.ascontiguousarray(pi[sel])).to(dev)
    act_d = torch.zeros(B, dtype=torch.int32, device=dev)
    stat_d = torch.zeros(B, dtype=torch.int32, device=dev)
    obs = torch.zeros((B, a.view, a.view, 3), dtype=torch.uint8, device=dev)
    direction = torch.zeros(B, dtype=torch.int32, device=dev)
    rew = torch.zeros(B, dtype=torch.float64, device=dev)
    term = torch.zeros(B, dtype=torch.uint8, device=dev)
    trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
    sstat = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(20):  # one stream: each lookup sees the step before it
        a.policy_actions_device(pi_d, 1, model, act_d, stat_d)
        a.step_device(act_d, obs, direction, rew, term, trunc, sstat)
    res = b.rollout(pi[sel], model=model, max_steps=20)
    sa, sb = a.get_state(), b.get_state()
    a.close()
    b.close()
    assert (res.steps == 20).all()
    for k in ("enc", "agent", "carry", "step_count"):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)


@pytest.mark.parametrize("name", ["lava9n2", "doorkey5"])
def test_zero_copy_from_a_solved_handle(name):
    import torch

    c = rr.case(name)
    enc, agent, model = c["enc"], c["agent"], c["model"]
    B = enc.shape[0]
    vi = mg.ValueIteration(enc, model=model, dtype="f64")
    vi.solve()
    _, pi_ptr = vi.device_buffers()
    assert pi_ptr
    dev = torch.device("cuda", 0)
    steps = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    ret = torch.zeros(B, dtype=torch.float64, device=dev)
    term = torch.zeros(B, dtype=torch.uint8, device=dev)
    trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
    tlen = 64
    ts = torch.zeros((tlen, B), dtype=torch.int32, device=dev)
    ta = torch.zeros((tlen, B), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    a = make_venv(c["env_id"], enc, agent)
    a.enable_timing(True)
    a.rollout_device(pi_ptr, 1, model, None, steps, ret, term, trunc, status, ts, ta, tlen)
    ms, launches = a.kernel_time()  # synchronises the handle's stream
    assert launches == 1 and ms > 0
    torch.cuda.synchronize()
    sa = a.get_state()
    a.close()
    pi = vi.policy()
    vi.close()
    b = make_venv(c["env_id"], enc, agent)
    res = b.rollout(pi, model=model, trace=True)
    sb = b.get_state()
    b.close()
    np.testing.assert_array_equal(steps.cpu().numpy(), res.steps)
    np.testing.assert_array_equal(ret.cpu().numpy(), res.ret)
    np.testing.assert_array_equal(term.cpu().numpy().astype(bool), res.terminated)
    np.testing.assert_array_equal(trunc.cpu().numpy().astype(bool), res.truncated)
    np.testing.assert_array_equal(status.cpu().numpy(), res.status)
    k = res.states.shape[0]
    assert 0 < k <= tlen
    np.testing.assert_array_equal(ts.cpu().numpy()[:k], res.states)
    np.testing.assert_array_equal(ta.cpu().numpy()[:k], res.actions)
    assert (ts.cpu().numpy()[k:] == -1).all()
    for key in ("enc", "agent", "carry", "step_count"):
        np.testing.assert_array_equal(sa[key], sb[key])
    # pi* reaches the goal from every solvable start and is checked against the reference too
    ref = rr.rollout_ref(enc, agent, pi, model, c["max_steps"], c["see_through"], trace_len=c["max_steps"])
    check(res, sb, ref, trace=True)
    assert res.terminated.any()


@pytest.mark.parametrize("name", ["lava9n2", "doorkey5"])
def test_bad_lanes_stop_only_their_env(name):
    """A lane of A (7 / 5) and a lane of -1 on a visited state: MGDP_E_ACTION there, the rest unaffected."""
    c = rr.case(name)
    pi, _ = rr.bad_policy(c)
    ref = rr.rollout_ref(c["enc"], c["agent"], pi, c["model"], c["max_steps"], c["see_through"])
    assert (ref["status"][[3, 7]] == _lib.MGDP_E_ACTION).all() and (np.delete(ref["status"], [3, 7]) == 0).all()
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    res = venv.rollout(pi, model=c["model"])
    check(res, venv.get_state(), ref)
    venv.close()
    assert not res.ok


def test_grids_and_carries_outside_the_model_are_refused_per_env():
    c = rr.case("lava9n2")
    enc, agent, pi = c["enc"].copy(), c["agent"], c["pi"]
    enc[2, 2, 1] = (6, 1, 0)  # a Ball next to env 2's start
    carry = np.zeros((65, 2), np.int32)
    carry[5] = (6, 1)  # env 5 carries a Ball
    ref = rr.rollout_ref(enc, agent, pi, "xyd", c["max_steps"], c["see_through"], carry=carry)
    assert (ref["status"][[2, 5]] == _lib.MGDP_E_UNSUPPORTED).all() and (ref["steps"][[2, 5]] == 0).all()
    assert (np.delete(ref["status"], [2, 5]) == 0).all()
    venv = make_venv(c["env_id"], enc, agent)
    _lib.check(venv.L.mgdp_envs_set_state(venv.h, None, _lib.ptr(carry), None, None), "mgdp_envs_set_state")
    res = venv.rollout(pi)
    check(res, venv.get_state(), ref)
    acts, status = venv.policy_actions(pi, return_status=True)
    assert (status[[2, 5]] == _lib.MGDP_E_UNSUPPORTED).all() and (acts[[2, 5]] == -1).all()
    # a DoorKey rollout of grids without a door: every env is outside the model
    dk = np.zeros((65, 16 * venv.W * venv.H), np.int8)
    res = venv.rollout(dk, model="doorkey")
    assert (res.status == _lib.MGDP_E_UNSUPPORTED).all() and (res.steps == 0).all()
    venv.close()
    # a DoorKey env that carries a Ball, and one with a second key
    d = rr.case("doorkey5")
    enc = d["enc"].copy()
    carry = np.zeros((65, 2), np.int32)
    carry[1] = (6, 1)
    free = np.argwhere(enc[4][..., 0] == 1)[-1]
    enc[4, free[0], free[1]] = (rr.KEY, 4, 0)
    ref = rr.rollout_ref(enc, d["agent"], d["pi"], "doorkey", d["max_steps"], d["see_through"], carry=carry)
    assert (ref["status"][[1, 4]] == _lib.MGDP_E_UNSUPPORTED).all()
    venv = make_venv(d["env_id"], enc, d["agent"])
    _lib.check(venv.L.mgdp_envs_set_state(venv.h, None, _lib.ptr(carry), None, None), "mgdp_envs_set_state")
    res = venv.rollout(d["pi"])
    check(res, venv.get_state(), ref)
    venv.close()
    # the C ABI's call-level refusals
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    out = [np.zeros(65, t) for t in (np.int32, np.float64, np.uint8, np.uint8, np.int32)]
    p = [_lib.ptr(o) for o in out]
    L, pp = venv.L, _lib.ptr(np.ascontiguousarray(pi))
    assert L.mgdp_envs_rollout(venv.h, 2, pp, 1, 0, *p, None, None, 0) == _lib.MGDP_E_INVALID
    assert L.mgdp_envs_rollout(venv.h, 0, pp, 0, 0, *p, None, None, 0) == _lib.MGDP_E_INVALID
    assert L.mgdp_envs_rollout(venv.h, 0, pp, 1, 0, *p, None, None, -1) == _lib.MGDP_E_INVALID
    assert L.mgdp_envs_policy_actions(venv.h, 0, pp, 0, p[0], p[4]) == _lib.MGDP_E_INVALID
    assert L.mgdp_envs_rollout(venv.h, 0, pp, 1, 0, *p, None, None, 0) == 0
    venv.close()


def test_call_level_errors_raise_value_error():
    c = rr.case("lava9n2")
    pi = c["pi"]
    venv = mg.MiniGridVecEnv(c["env_id"], 65, autoreset=True)
    venv.load(c["enc"], c["agent"])
    with pytest.raises(ValueError):
        venv.rollout(pi)
    with pytest.raises(ValueError):
        venv.policy_actions(pi)
    venv.close()
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    for bad in (pi[:64], pi[:, :-1], pi.astype(np.float32), pi[None], pi.astype(np.int32) + 1000,
                np.zeros((2, 64, pi.shape[1]), np.int8)):
        with pytest.raises(ValueError):
            venv.rollout(bad)
    with pytest.raises(ValueError):
        venv.rollout(pi, model="xyz")
    with pytest.raises(ValueError):
        venv.rollout(pi, model="doorkey")  # (B, 4*W*H) is not the DoorKey model's shape
    with pytest.raises(ValueError):
        venv.rollout(pi, max_steps=0)
    res = venv.rollout(mg.VIResult(None, pi, 0, True, 0.0, "xyd", venv.W, venv.H), max_steps=5)  # a VIResult's pi and model
    np.testing.assert_array_equal(res.steps, np.minimum(c["ref"]["steps"], 5))
    venv.set_contents(np.zeros((65, venv.W, venv.H, 3), np.uint8))
    with pytest.raises(ValueError):
        venv.rollout(pi)
    # the C ABI refuses the handle too, whatever the Python front end remembers
    out = [np.zeros(65, t) for t in (np.int32, np.float64, np.uint8, np.uint8, np.int32)]
    rc = venv.L.mgdp_envs_rollout(venv.h, 0, _lib.ptr(np.ascontiguousarray(pi)), 1, 0, *[_lib.ptr(o) for o in out],
                                  None, None, 0)
    assert rc == _lib.MGDP_E_UNSUPPORTED
    venv.close()


@pytest.mark.parametrize("knob", [{"MGDP_ROLLOUT_READER": "hbm"}])
@pytest.mark.parametrize("name", ["lava9n2", "doorkey5"])
def test_the_ab_sides_compute_the_same(name, knob, monkeypatch):
    """The cell reader in HBM on grids that fit LDS: read at handle creation, the same results
    (tools/probe_rollout.py times the two)."""
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    c = rr.case(name)
    res, st = run_case(c, trace=True)
    check(res, st, c["ref"], trace=True)
    monkeypatch.setenv("MGDP_ROLLOUT_READER", "neither")
    with pytest.raises(ValueError):
        mg.MiniGridVecEnv(c["env_id"], 1)
