"""Tabular Q-learning on resident envs (csrc/envs_qlearn.h) against the host restatement
tests/qlearn_ref.py: Q, steps, episodes, wins, fp64 return, status and trace array-equal, both streams' records
against numpy's own state integers, and get_state() after the call equal to get_state() before it.  Each
_case_* function builds its inputs and the restatement's result on the host and asserts there what the case is
meant to contain."""
import os
import subprocess
import sys

import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from tests import qlearn_ref as qr
from tests import rollout_ref as rr
from tests import slip_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("enc", "agent", "carry", "step_count")
KEY = rr.KEY


def check_streams(got, streams):
    want = sr.stream_fields(streams) if isinstance(streams, list) else streams
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def check(res, ref, trace=True):
    """Every output of q_learn against the restatement's."""
    np.testing.assert_array_equal(res.status, ref["status"])
    np.testing.assert_array_equal(res.steps, ref["steps"])
    np.testing.assert_array_equal(res.episodes, ref["episodes"])
    np.testing.assert_array_equal(res.wins, ref["wins"])
    np.testing.assert_array_equal(res.ret, ref["ret"])
    np.testing.assert_array_equal(res.Q, ref["Q"])
    if trace:
        np.testing.assert_array_equal(res.states, ref["states"])
        np.testing.assert_array_equal(res.actions, ref["actions"])


def learn(venv, n_steps, ref=None, slip=False, trace=True, **kw):
    """One q_learn call between two get_state() reads; everything checked against ref."""
    before = venv.get_state()
    res = venv.q_learn(n_steps, trace=trace, **kw)
    after = venv.get_state()
    for k in STATE_KEYS:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    if ref is not None:
        check(res, ref, trace=bool(trace))
        check_streams(venv.explore_streams(), ref["streams"])
        if slip:
            check_streams(venv.slip_streams(), ref["slip_streams"])
    return res


def make_venv(env_id, enc, agent, max_steps=None, **kw):
    venv = mg.MiniGridVecEnv(env_id, enc.shape[0], **kw)
    venv.load(enc, agent, max_steps=max_steps)
    return venv


_CASES: dict = {}


def cached(fn):
    def wrapper(*a):
        key = (fn.__name__,) + a
        if key not in _CASES:
            _CASES[key] = fn(*a)
        return _CASES[key]
    return wrapper


# ---------------------------------------------------------------------------------------------- 1
@cached
def _case_empty5(n_act, eps):
    enc, agent, env = rr.grids("MiniGrid-Empty-5x5-v0", 3)
    ref = qr.qlearn_ref(enc, agent, "xyd", env.max_steps, 300, eps=eps, n_act=n_act, seed0=3, trace_len=300)
    assert (ref["steps"] == 300).all()
    if eps == 0:
        assert (ref["int_calls"] == 0).all()  # no integers() call ever happens
    if eps == 1:
        assert (ref["int_calls"] == 300).all()
    return enc, agent, env.max_steps, ref


@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n_act", [3, 7])
def test_empty5_partial_wave(n_act, eps):
    enc, agent, ms, ref = _case_empty5(n_act, eps)
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    learn(venv, 300, ref, eps=eps, n_act=n_act, seed=3)
    venv.close()


# ---------------------------------------------------------------------------------------------- 2
@cached
def _case_lava(nodeath):
    env_id, dc = "MiniGrid-LavaCrossingS9N1-v0", -0.75
    enc, agent, env = rr.grids(env_id, 65)
    kw = dict(nd_types=("lava",), death_cost=dc) if nodeath else {}
    ref = qr.qlearn_ref(enc, agent, "xyd", env.max_steps, 400, eps=0.5, n_act=3, seed0=0, trace_len=400,
                        see_through=env.see_through_walls, **kw)
    assert (ref["episodes"] >= 1).all(), "every env restarts at least once"
    terms = np.bincount([e["env"] for e in ref["episodes_log"] if e["end"] == "term"], minlength=65)
    if nodeath:  # lava costs and the episode goes on: only the goal terminates
        np.testing.assert_array_equal(terms, ref["wins"])
        assert (ref["ret"] < dc).any(), "no env paid the death cost"
    else:
        assert (terms > ref["wins"]).any(), "no lava termination"
    return env_id, enc, agent, dc, ref


def test_lava_two_waves_many_restarts():
    env_id, enc, agent, dc, ref = _case_lava(False)
    venv = make_venv(env_id, enc, agent)
    learn(venv, 400, ref, eps=0.5, n_act=3, seed=0)
    venv.close()


def test_nodeath_lava():
    env_id, enc, agent, dc, ref = _case_lava(True)
    venv = make_venv(env_id, enc, agent, no_death_types=("lava",), death_cost=dc)
    learn(venv, 400, ref, eps=0.5, n_act=3, seed=0)
    venv.close()


# ---------------------------------------------------------------------------------------------- 3
@cached
def _case_doorkey(size):
    env_id = f"MiniGrid-DoorKey-{size}x{size}-v0"
    enc, agent, env = rr.grids(env_id, 65)
    ref = qr.qlearn_ref(enc, agent, "doorkey", 20, 600, eps=1.0, seed0=0, trace_len=600,
                        see_through=env.see_through_walls)
    log = ref["episodes_log"]
    assert any(e["picked"] and e["end"] == "trunc" for e in log), "no key picked up inside a truncated episode"
    assert any(e["opened"] and e["end"] == "trunc" for e in log), "no door opened inside a truncated episode"
    assert (ref["trunc_bootstraps"] > 0).all()
    return env_id, enc, agent, ref


@pytest.mark.parametrize("size", [5, 8])
def test_doorkey_plane_restore(size):
    """max_steps = 20 and uniform lanes: episodes that picked the key up or opened the door are truncated, and the
    next one starts on the snapshot's plane again."""
    env_id, enc, agent, ref = _case_doorkey(size)
    venv = make_venv(env_id, enc, agent, max_steps=20)
    learn(venv, 600, ref, eps=1.0, seed=0)
    venv.close()


# ---------------------------------------------------------------------------------------------- 4
@cached
def _case_snapshot():
    env_id = "MiniGrid-DoorKey-5x5-v0"
    enc, agent, env = rr.grids(env_id, 65)
    enc = enc.copy()
    carry = np.zeros((65, 2), np.int32)
    for b in range(65):  # the key is in the agent's hands, not on the grid
        (kx, ky), = np.argwhere(enc[b, :, :, 0] == KEY)
        carry[b] = (KEY, enc[b, kx, ky, 1])
        enc[b, kx, ky] = (1, 0, 0)
    sc = np.full(65, 7, np.int32)
    ref = qr.qlearn_ref(enc, agent, "doorkey", 30, 300, eps=0.6, seed0=9, trace_len=300, carry=carry, step_count=sc,
                        see_through=env.see_through_walls)
    assert (ref["status"] == 0).all() and (ref["episodes"] >= 300 // 23).all()
    assert any(e["opened"] for e in ref["episodes_log"]), "no env opened the door with the key it entered with"
    # every episode restarts with the key carried: state index has_key set at each episode's first step
    assert ((ref["states"][0] >> 1) & 1).all()
    return env_id, enc, agent, carry, sc, ref


def test_entry_from_a_non_reset_snapshot():
    env_id, enc, agent, carry, sc, ref = _case_snapshot()
    venv = make_venv(env_id, enc, agent, max_steps=30)
    mg._lib.check(venv.L.mgdp_envs_set_state(venv.h, None, mg._lib.ptr(carry), mg._lib.ptr(sc), None), "mgdp_envs_set_state")
    st = venv.get_state()
    np.testing.assert_array_equal(st["carry"], carry)
    np.testing.assert_array_equal(st["step_count"], sc)
    learn(venv, 300, ref, eps=0.6, seed=9)
    venv.close()


# ---------------------------------------------------------------------------------------------- 5
@cached
def _case_optimistic():
    enc, agent, env = rr.grids("MiniGrid-Empty-6x6-v0", 3)
    Q0 = np.ones((3, 6 * 6 * 4, 7))
    ref = qr.qlearn_ref(enc, agent, "xyd", env.max_steps, 300, Q=Q0, eps=0.05, alpha=0.25, gamma=0.95, seed0=2,
                        trace_len=300)
    assert len(np.unique(ref["actions"])) == 7  # optimism tries every lane
    return enc, agent, Q0, ref


def test_optimistic_start():
    enc, agent, Q0, ref = _case_optimistic()
    venv = make_venv("MiniGrid-Empty-6x6-v0", enc, agent)
    keep = Q0.copy()
    learn(venv, 300, ref, Q=Q0, eps=0.05, alpha=0.25, gamma=0.95, seed=2)
    np.testing.assert_array_equal(Q0, keep)  # the caller's table is not written
    venv.close()


# ---------------------------------------------------------------------------------------------- 6
@cached
def _case_continuation(seed0):
    enc, agent, env = rr.grids("MiniGrid-Empty-5x5-v0", 3)
    ms = env.max_steps
    ref1 = qr.qlearn_ref(enc, agent, "xyd", ms, 41, eps=0.5, n_act=3, seed0=seed0, trace_len=41)
    half = [b for b in range(3) if ref1["streams"][b]["has_uint32"] == 1]
    assert half, "no env ends the first call with a buffered half-word"
    ref2 = qr.qlearn_ref(enc, agent, "xyd", ms, 259, Q=ref1["Q"], eps=0.5, n_act=3, rngs=ref1["rngs"], trace_len=259)
    assert all(ref2["int_calls"][b] > 0 for b in half)  # ... and goes on to use it
    return enc, agent, ref1, ref2


@pytest.mark.parametrize("seed0", [0, 2**32 - 2])
def test_continuing_call_and_seed_words(seed0):
    """seed=None continues Q's streams (half-word buffer included) and starts a new episode at the snapshot.
    SeedSequence takes 2^32 - 2 and 2^32 - 1 as one 32-bit word and 2^32 as two."""
    enc, agent, ref1, ref2 = _case_continuation(seed0)
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    venv.set_explore(seed0)
    check_streams(venv.explore_streams(), sr.fresh_streams(seed0, 3))
    r1 = learn(venv, 41, ref1, eps=0.5, n_act=3, seed=seed0)
    learn(venv, 259, ref2, Q=r1.Q, eps=0.5, n_act=3)
    venv.close()


def test_first_use_without_a_seed_is_seed_zero():
    enc, agent, ms, ref = _case_empty5(3, 0.3)
    ref0 = qr.qlearn_ref(enc, agent, "xyd", ms, 50, eps=0.3, n_act=3, seed0=0, trace_len=50)
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    learn(venv, 50, ref0, eps=0.3, n_act=3)
    venv.close()


# ---------------------------------------------------------------------------------------------- 7
@cached
def _case_slip(model):
    if model == "xyd":
        env_id, ms, n, kw = "MiniGrid-LavaCrossingS9N1-v0", None, 300, dict(eps=0.3, n_act=3)
    else:
        env_id, ms, n, kw = "MiniGrid-DoorKey-5x5-v0", 40, 400, dict(eps=0.8)
    enc, agent, env = rr.grids(env_id, 65)
    ref = qr.qlearn_ref(enc, agent, model, ms or env.max_steps, n, seed0=1, trace_len=n, slip=(0.7, None), slip_seed0=5,
                        see_through=env.see_through_walls, **kw)
    lanes = (0, 1, 2) if model == "xyd" else (0, 1, 2, 3, 5)
    assert (~np.isin(ref["actions"], lanes)).any(), "no slipped action outside the learner's lanes"
    if model == "doorkey":  # drop is no lane of the model: only a slip executes it
        assert any(e["dropped"] for e in ref["episodes_log"]), "no slipped drop mutated a plane"
    return env_id, enc, agent, ms, n, kw, ref


@pytest.mark.parametrize("model", ["xyd", "doorkey"])
def test_slip_on_the_handle(model):
    env_id, enc, agent, ms, n, kw, ref = _case_slip(model)
    venv = make_venv(env_id, enc, agent, max_steps=ms)
    venv.set_slip(0.7, seed=5)
    learn(venv, n, ref, slip=True, seed=1, **kw)
    venv.close()


# ---------------------------------------------------------------------------------------------- 8
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import minigrid_dynamicprogramming_amd as mg
d = np.load(sys.argv[2])
venv = mg.MiniGridVecEnv("MiniGrid-LavaCrossingS9N1-v0", d["enc"].shape[0])
venv.load(d["enc"], d["agent"])
res = venv.q_learn(400, eps=0.5, n_act=3, seed=0, trace=True)
st = venv.get_state()
np.savez(sys.argv[3], Q=res.Q, steps=res.steps, episodes=res.episodes, wins=res.wins, ret=res.ret, status=res.status,
         states=res.states, actions=res.actions, enc=st["enc"], agent=st["agent"], carry=st["carry"],
         step_count=st["step_count"])
venv.close()
print("child ok")
"""


@pytest.mark.parametrize("reader", ["hbm", "lds"])
def test_both_readers_in_a_child_process(reader, tmp_path):
    """MGDP_ROLLOUT_READER is read when the handle is created: a fresh process with the knob set."""
    env_id, enc, agent, dc, ref = _case_lava(False)
    np.savez(tmp_path / "in.npz", enc=enc, agent=agent)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, MGDP_ROLLOUT_READER=reader))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    out = np.load(tmp_path / "out.npz")
    for k in ("Q", "steps", "episodes", "wins", "ret", "status", "states", "actions"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(out["enc"], enc)
    np.testing.assert_array_equal(out["agent"], agent)
    assert not out["carry"].any() and not out["step_count"].any()


@cached
def _case_big_empty():
    enc, agent, env = rr.grids("MiniGrid-Empty-5x5-v0", 2, size=52)
    assert 64 * ((52 * 52 + 15) // 16 * 16 + 4) > 160 * 1024 - 2048  # above the LDS limit: the HBM reader
    ref = qr.qlearn_ref(enc, agent, "xyd", env.max_steps, 200, eps=0.4, n_act=3, seed0=0, trace_len=200)
    return enc, agent, ref


def test_xyd_above_the_lds_limit_runs_on_the_hbm_reader():
    enc, agent, ref = _case_big_empty()
    venv = mg.MiniGridVecEnv("MiniGrid-Empty-5x5-v0", 2, size=52)
    venv.load(enc, agent)
    learn(venv, 200, ref, eps=0.4, n_act=3, seed=0)
    venv.close()


def test_doorkey_above_the_lds_limit_is_unsupported():
    enc, agent, env = rr.grids("MiniGrid-DoorKey-5x5-v0", 2, size=52)
    venv = mg.MiniGridVecEnv("MiniGrid-DoorKey-5x5-v0", 2, size=52)
    venv.load(enc, agent)
    with pytest.raises(ValueError, match="LDS"):
        venv.q_learn(10, seed=0)
    assert mg._lib.MGDP_E_UNSUPPORTED == -3
    venv.close()


# ---------------------------------------------------------------------------------------------- 9
@cached
def _case_box():
    enc, agent, env = rr.grids("MiniGrid-Empty-6x6-v0", 8)
    enc = enc.copy()
    enc[3, 3, 2] = (7, 2, 0)  # a Box: outside the XYD model
    Q0 = np.random.default_rng(7).uniform(-1, 1, (8, 6 * 6 * 4, 7))
    ref = qr.qlearn_ref(enc, agent, "xyd", env.max_steps, 120, Q=Q0, eps=0.3, seed0=4, trace_len=120)
    assert ref["status"].tolist() == [0, 0, 0, rr.E_UNSUPPORTED, 0, 0, 0, 0] and ref["steps"][3] == 0
    assert (ref["states"][:, 3] == -1).all()
    return enc, agent, Q0, ref


def test_an_env_outside_the_model_is_refused_alone():
    enc, agent, Q0, ref = _case_box()
    venv = make_venv("MiniGrid-Empty-6x6-v0", enc, agent)
    res = learn(venv, 120, ref, Q=Q0, eps=0.3, seed=4)
    assert res.status[3] == mg._lib.MGDP_E_UNSUPPORTED and not res.ok
    assert res.Q[3].tobytes() == Q0[3].tobytes()  # bit-unchanged rows
    fresh = sr.fresh_streams(4, 8)
    got = venv.explore_streams()
    for k in fresh:
        assert got[k][3] == fresh[k][3], k  # an unadvanced stream
    venv.close()


# ---------------------------------------------------------------------------------------------- 10
def test_refusals():
    enc, agent, ms, _ = _case_empty5(3, 0.3)
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    S = 5 * 5 * 4
    with pytest.raises(ValueError):
        venv.explore_streams()  # before any seeding
    dummy = np.zeros(3, np.int32)
    retd = np.zeros(3, np.float64)
    with pytest.raises(ValueError):  # MGDP_E_INVALID: continuing (no seed) before any seeding; the pointers are never used
        venv.q_learn_device(0, 10, "xyd", 0, 0, 0, 0, 0)
    L, p, h = venv.L, mg._lib.ptr, venv.h
    Q = np.zeros((3, S, 7))
    outs = (p(dummy), p(dummy.copy()), p(dummy.copy()), p(retd), p(dummy.copy()), None, None, 0)
    assert L.mgdp_envs_q_learn(h, 0, p(Q), 10, 0.5, 0.9, 0.1, 3, 0, *outs) == mg._lib.MGDP_E_INVALID
    with pytest.raises(ValueError):
        venv.set_explore(0, mask=np.ones(3, np.uint8))  # a masked first call
    venv.set_explore(0)
    bad = [dict(n_steps=0), dict(n_steps=-3), dict(n_act=0), dict(n_act=8), dict(eps=-0.1), dict(eps=1.5),
           dict(eps=float("nan")), dict(alpha=float("nan")), dict(gamma=float("nan"))]
    for kw in bad:
        a = dict(n_steps=10, alpha=0.5, gamma=0.9, eps=0.1, n_act=3)
        a.update(kw)
        with pytest.raises(ValueError):
            venv.q_learn(a["n_steps"], alpha=a["alpha"], gamma=a["gamma"], eps=a["eps"], n_act=a["n_act"])
        # the C entry refuses the same arguments itself
        rc = L.mgdp_envs_q_learn(h, 0, p(Q), a["n_steps"], a["alpha"], a["gamma"], a["eps"], a["n_act"], 0, *outs)
        assert rc == mg._lib.MGDP_E_INVALID, kw
    assert L.mgdp_envs_q_learn(h, 1, p(Q), 10, 0.5, 0.9, 0.1, 6, 0, *outs) == mg._lib.MGDP_E_INVALID  # DoorKey: A = 5
    assert L.mgdp_envs_q_learn(h, 0, p(Q), 10, 0.5, 0.9, 0.1, 3, 2, *outs) == mg._lib.MGDP_E_INVALID  # unit_goal
    assert not Q.any()
    for Qbad in (np.zeros((3, S, 7), np.float32), np.zeros((3, S, 5)), np.zeros((2, S, 7)), np.zeros((3, S))):
        with pytest.raises(ValueError):
            venv.q_learn(10, Q=Qbad)
        with pytest.raises(ValueError):
            venv.q_greedy(Qbad)
    with pytest.raises(ValueError):
        venv.q_learn(10, model="nope")
    with pytest.raises(ValueError):
        venv.q_learn(10, trace=-1)
    with pytest.raises(ValueError):
        venv.q_greedy(Q, n_act=0)
    check_streams(venv.explore_streams(), sr.fresh_streams(0, 3))  # no refused call drew anything
    venv.close()
    venv = mg.MiniGridVecEnv("MiniGrid-Empty-5x5-v0", 3, autoreset=True)
    venv.load(enc, agent)
    with pytest.raises(ValueError):
        venv.q_learn(10)
    with pytest.raises(ValueError):
        venv.q_greedy(Q)
    venv.close()
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    venv.set_contents(np.zeros((3, 5, 5, 3), np.uint8))  # Box contents planes on the handle
    with pytest.raises(ValueError):
        venv.q_learn(10)
    venv.set_explore(0)
    assert L.mgdp_envs_q_learn(venv.h, 0, p(Q), 10, 0.5, 0.9, 0.1, 3, 0, *outs) == mg._lib.MGDP_E_UNSUPPORTED
    venv.close()


# ---------------------------------------------------------------------------------------------- 11
def test_q_greedy_against_numpy_with_ties():
    rng = np.random.default_rng(0)
    for env_id, model, A in (("MiniGrid-Empty-5x5-v0", "xyd", 7), ("MiniGrid-DoorKey-5x5-v0", "doorkey", 5)):
        enc, agent, env = rr.grids(env_id, 3)
        S = qr.n_states(model, 5, 5)
        Q = rng.integers(-2, 3, (3, S, A)).astype(np.float64)  # few distinct values: ties in most rows
        Q[0, :7] = 0.0
        Q[1] += rng.normal(size=(S, A)) * (rng.random((S, 1)) < 0.5)
        venv = make_venv(env_id, enc, agent)
        for n_act in (1, 3, A):
            pi, vq = venv.q_greedy(Q, n_act=n_act, values=True)
            assert pi.dtype == np.int8 and pi.shape == (3, S) and vq.shape == (3, S)
            np.testing.assert_array_equal(pi, np.argmax(Q[..., :n_act], axis=-1))
            np.testing.assert_array_equal(vq, np.max(Q[..., :n_act], axis=-1))
        np.testing.assert_array_equal(venv.q_greedy(Q), np.argmax(Q, axis=-1))
        venv.close()


def test_rollout_of_the_greedy_table():
    """q_learn -> q_greedy -> rollout(pi) against rollout_ref on the learned table."""
    env_id, enc, agent, dc, ref = _case_lava(False)
    venv = make_venv(env_id, enc, agent)
    pi, vq = venv.q_greedy(ref["Q"], n_act=3, values=True)
    want_pi, want_v = qr.greedy_ref(ref["Q"], 3)
    np.testing.assert_array_equal(pi, want_pi)
    np.testing.assert_array_equal(vq, want_v)
    res = venv.rollout(pi, model="xyd")
    env = mg.make(env_id)
    want = rr.rollout_ref(enc, agent, want_pi, "xyd", env.max_steps, env.see_through_walls)
    np.testing.assert_array_equal(res.steps, want["steps"])
    np.testing.assert_array_equal(res.ret, want["ret"])
    np.testing.assert_array_equal(res.terminated, want["terminated"])
    np.testing.assert_array_equal(res.truncated, want["truncated"])
    venv.close()


def test_device_entry_on_torch_tensors():
    import torch

    env_id, enc, agent, ref = _case_doorkey(5)
    B, S, A = 65, qr.n_states("doorkey", 5, 5), 5
    venv = make_venv(env_id, enc, agent, max_steps=20)
    venv.set_explore(0)
    dev = torch.device("cuda", 0)
    Q = torch.zeros((B, S, A), dtype=torch.float64, device=dev)
    steps, episodes, wins, status = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    ret = torch.zeros(B, dtype=torch.float64, device=dev)
    ts = torch.zeros((600, B), dtype=torch.int32, device=dev)
    ta = torch.zeros((600, B), dtype=torch.int8, device=dev)
    pi = torch.zeros((B, S), dtype=torch.int8, device=dev)
    vq = torch.zeros((B, S), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    venv.q_learn_device(Q, 600, "doorkey", steps, episodes, wins, ret, status, eps=1.0, trace_state=ts, trace_action=ta,
                        trace_len=600)
    venv.q_greedy_device(Q, "doorkey", pi, vq)
    streams = venv.explore_streams()  # synchronises the handle's stream
    res = mg.QLearnResult(Q.cpu().numpy(), steps.cpu().numpy(), episodes.cpu().numpy(), wins.cpu().numpy(),
                          ret.cpu().numpy(), status.cpu().numpy(), ts.cpu().numpy(), ta.cpu().numpy())
    check(res, ref)
    check_streams(streams, ref["streams"])
    want_pi, want_v = qr.greedy_ref(ref["Q"], A)
    np.testing.assert_array_equal(pi.cpu().numpy(), want_pi)
    np.testing.assert_array_equal(vq.cpu().numpy(), want_v)
    venv.close()


# ---------------------------------------------------------------------------------------------- 12
@pytest.mark.parametrize("name", list(qr.TIE))
def test_dp_tie(name):
    """eps = 1, alpha = 1, unit_goal, gamma = 0.9, Q = 0, seed 0: the learner reproduces the oracle's V* to
    1e-12 on the checked states, equals the restatement bit for bit, and its greedy table's rollout reaches the
    goal in the oracle's optimal step count in all 8 envs."""
    c = qr.tie_case(name)
    venv = make_venv(c["env_id"], c["enc"], c["agent"])
    res = learn(venv, c["n_steps"], c["ref"], trace=False, model=c["model"], alpha=1.0, gamma=qr.TIE_GAMMA, eps=1.0,
                n_act=c["n_act"], unit_goal=True, seed=0)
    err = qr.tie_error(c, res.Q)
    print(f"{name}: max |max_a Q - V*| = {err:.3e}")
    assert err <= qr.TIE_TOL
    pi, vq = venv.q_greedy(res.Q, model=c["model"], n_act=c["n_act"], values=True)
    assert float(np.abs(vq - c["V"])[c["on"]].max()) <= qr.TIE_TOL
    got = venv.rollout(pi, model=c["model"])
    assert got.ok and got.terminated.all() and (got.ret > 0).all()
    np.testing.assert_array_equal(got.steps, c["opt_steps"])
    venv.close()


# ---------------------------------------------------------------------------------------------- 13
def test_masked_explore_reseed_after_a_first_seeding():
    """set_explore(mask=...) after the streams were seeded and used: the masked envs get default_rng(seed + b),
    the others keep their records as the learner left them."""
    enc, agent, env = rr.grids("MiniGrid-Empty-5x5-v0", 3)
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    venv.set_explore(7)
    venv.q_learn(20)
    before = venv.explore_streams()
    first = sr.fresh_streams(7, 3)
    assert all(before["state"][b] != first["state"][b] for b in range(3)), "a stream that q_learn did not advance"
    mask = np.array([1, 0, 1], np.uint8)
    venv.set_explore(100, mask=mask)
    got = venv.explore_streams()
    venv.close()
    fresh = sr.fresh_streams(100, 3)  # env b: default_rng(100 + b)
    for k in fresh:
        assert got[k][0] == fresh[k][0] and got[k][2] == fresh[k][2], k
        assert got[k][1] == before[k][1], k
    check_streams(got, {k: np.where(mask.astype(bool), fresh[k], before[k]) for k in fresh})


def test_one_trace_buffer_given():
    """A trace needs both of its buffers.  The device entries refuse one alone and write nothing; the host
    entries refuse one alone with trace_len > 0 and take no trace with trace_len == 0."""
    import torch

    INVALID = mg._lib.MGDP_E_INVALID
    enc, agent, env = rr.grids("MiniGrid-Empty-5x5-v0", 3)
    venv = make_venv("MiniGrid-Empty-5x5-v0", enc, agent)
    venv.set_explore(7)
    L, p, h = venv.L, mg._lib.ptr, venv.h
    B, S, A, n = 3, 5 * 5 * 4, 7, 4
    dev = torch.device("cuda", 0)
    Q = torch.zeros((B, S, A), dtype=torch.float64, device=dev)
    pi = torch.zeros((B, S), dtype=torch.int8, device=dev)
    i32 = [torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(4)]
    ret = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
    u8 = [torch.full((B,), 9, dtype=torch.uint8, device=dev) for _ in range(2)]
    ts = torch.full((n, B), -7, dtype=torch.int32, device=dev)
    ta = torch.full((n, B), -7, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    state0, streams0 = venv.get_state(), venv.explore_streams()
    for s, a in ((p(ts), None), (None, p(ta))):
        rc = L.mgdp_envs_rollout_device(h, 0, p(pi), 1, 5, p(i32[0]), p(ret), p(u8[0]), p(u8[1]), p(i32[1]), s, a, n)
        assert rc == INVALID
        rc = L.mgdp_envs_q_learn_device(h, 0, p(Q), 10, 0.5, 0.9, 0.1, 3, 0, p(i32[0]), p(i32[1]), p(i32[2]), p(ret),
                                        p(i32[3]), s, a, n)
        assert rc == INVALID
    streams1, state1 = venv.explore_streams(), venv.get_state()  # synchronises the handle's stream
    torch.cuda.synchronize()
    assert not Q.any().item()
    assert all((t == -7).all().item() for t in i32 + [ret, ts, ta]) and all((t == 9).all().item() for t in u8)
    check_streams(streams1, streams0)
    for k in STATE_KEYS:
        np.testing.assert_array_equal(state1[k], state0[k], err_msg=k)
    # the host entries
    hQ, hpi = np.zeros((B, S, A)), np.zeros((B, S), np.int8)
    hi32 = [np.full(B, -7, np.int32) for _ in range(4)]
    hret = np.full(B, -7.0)
    hu8 = [np.full(B, 9, np.uint8) for _ in range(2)]
    hts, hta = np.full((n, B), -7, np.int32), np.full((n, B), -7, np.int8)

    def rollout(s, a, tlen):
        return L.mgdp_envs_rollout(h, 0, p(hpi), 1, 5, p(hi32[0]), p(hret), p(hu8[0]), p(hu8[1]), p(hi32[1]), s, a, tlen)

    def q_learn(s, a, tlen):
        return L.mgdp_envs_q_learn(h, 0, p(hQ), 10, 0.5, 0.9, 0.1, 3, 0, p(hi32[0]), p(hi32[1]), p(hi32[2]), p(hret),
                                   p(hi32[3]), s, a, tlen)

    for s, a in ((p(hts), None), (None, p(hta))):
        assert rollout(s, a, n) == INVALID
        assert q_learn(s, a, n) == INVALID
    assert not hQ.any() and all((t == -7).all() for t in hi32 + [hret]) and all((t == 9).all() for t in hu8)
    check_streams(venv.explore_streams(), streams0)
    for s, a in ((p(hts), None), (None, p(hta))):
        assert rollout(s, a, 0) == 0
        assert (hi32[0] == 5).all() and (hi32[1] == 0).all()  # five steps each, status ok
        assert q_learn(s, a, 0) == 0
        assert (hi32[0] == 10).all() and (hi32[3] == 0).all()
    assert (hts == -7).all() and (hta == -7).all()  # no trace was taken
    venv.close()
