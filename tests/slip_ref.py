"""Host restatement of the slip rollout of DESIGN.md section 17: the section 16 loop of tests/rollout_ref.py
with one slip decision between the policy lookup and the step.

Env b draws from numpy.random.default_rng(seed0 + b) -- numpy itself, not a restatement of it -- and steps
through oracle.OracleEnv.step, so the GPU rollout has a reference that shares no code with it.  Besides what
rr.rollout_ref returns, the dict holds each env's final bit_generator.state ("streams"), the generators
themselves ("rngs", which a continuing call takes over) and what the tests assert about their own inputs:
"slipped" (trace_len, B), "int_draw_steps" (per env, the steps at which integers() was called) and "events"
(one per slipped pickup / drop / toggle).
"""
from __future__ import annotations

import numpy as np

from minigrid_dynamicprogramming_amd.core import OBJECT_TO_IDX
from minigrid_dynamicprogramming_amd.dp import DOORKEY_ACTIONS, n_actions, state_index
from oracle.oracle import OracleEnv
from tests import rollout_ref as rr

PICKUP, DROP, TOGGLE = 3, 4, 5


def slip_decide(rng, prob, random_action, a):
    """One slip decision: (the executed action, whether it was replaced, whether integers() was called)."""
    if rng.random() < prob:
        return a, False, False
    if random_action is not None:
        return int(random_action), True, False
    return int(rng.integers(0, 6)), True, True


def slip_rollout_ref(enc, agent, pi, model, max_steps, prob, seed0=0, random_action=None, see_through=False,
                     carry=None, step_count=None, n_max=0, trace_len=0, nd_types=(), death_cost=-1.0, rngs=None):
    """rr.rollout_ref's arguments plus prob, seed0 and random_action (None: a draw of 0..5).  rngs: the
    generators a previous call returned, instead of fresh ones of seed0 + b."""
    enc = np.asarray(enc, np.uint8)
    B, W = enc.shape[0], enc.shape[1]
    pi = np.asarray(pi)
    T = 1 if pi.ndim == 2 else pi.shape[0]
    pit = pi[None] if pi.ndim == 2 else pi
    A = n_actions(model)
    ms = np.broadcast_to(np.asarray(max_steps, np.int32), (B,))
    if rngs is None:
        rngs = [np.random.default_rng(seed0 + b) for b in range(B)]
    out = {"steps": np.zeros(B, np.int32), "ret": np.zeros(B, np.float64), "terminated": np.zeros(B, bool),
           "truncated": np.zeros(B, bool), "status": np.zeros(B, np.int32),
           "states": np.full((trace_len, B), -1, np.int32), "actions": np.full((trace_len, B), -1, np.int8),
           "slipped": np.zeros((trace_len, B), bool), "int_draw_steps": [[] for _ in range(B)], "events": [],
           "enc": enc.copy(), "agent": np.zeros((B, 3), np.int32), "carry": np.zeros((B, 2), np.int32),
           "step_count": np.zeros(B, np.int32), "rngs": rngs}
    nd = tuple(OBJECT_TO_IDX[t] for t in nd_types)
    for b in range(B):
        o = OracleEnv(enc[b], agent[b], int(ms[b]), see_through)
        rng = rngs[b]
        if carry is not None:
            o.carry[:] = carry[b]
        if step_count is not None:
            o.state[3] = step_count[b]
        status = rr.model_status(model, enc[b], o.carry)  # at entry only
        door = np.argwhere(enc[b, :, :, 0] == rr.DOOR)
        n, ret, te, tr = 0, 0.0, False, False
        while status == rr.OK and (n_max <= 0 or n < n_max):
            x, y, d, sc = (int(v) for v in o.state)
            hk = dop = 0
            if model == "doorkey":
                hk = int(o.carry[0] == rr.KEY)
                dop = int(o.st[door[0][1], door[0][0]] == 0)
            s = state_index(model, W, x, y, d, hk, dop)
            if T > 1 and not 0 <= sc < T:
                status = rr.E_INVALID  # a failed lookup draws nothing
                break
            lane = int(pit[sc if T > 1 else 0, b, s])
            if not 0 <= lane < A:
                status = rr.E_ACTION
                break
            a = DOORKEY_ACTIONS[lane] if model == "doorkey" else lane
            a, slipped, drew = slip_decide(rng, prob, random_action, a)
            if drew:
                out["int_draw_steps"][b].append(n)
            fx, fy = x + rr.DIRS[d][0], y + rr.DIRS[d][1]
            if not (0 <= fx < W and 0 <= fy < o.H):  # the env as it was, the stream advanced
                status = rr.E_BOUNDS
                break
            going = a == 2 and o.ty[fy, fx] in nd
            watch = slipped and a in (PICKUP, DROP, TOGGLE)
            before = (o.ty[fy, fx], o.co[fy, fx], o.st[fy, fx]) if watch else None
            _, r, te, tr = o.step(a)
            if watch:
                out["events"].append({"env": b, "step": n, "action": a, "had_key": bool(hk),
                                      "changed": before != (o.ty[fy, fx], o.co[fy, fx], o.st[fy, fx])})
            in_death = o.ty[o.state[1], o.state[0]] in nd
            if nd and te and (going or in_death):
                te, r = False, r + death_cost
            if n < trace_len:
                out["states"][n, b], out["actions"][n, b], out["slipped"][n, b] = s, a, slipped
            n += 1
            ret = ret + r
            if te or tr:
                break
        out["steps"][b], out["ret"][b], out["terminated"][b], out["truncated"][b], out["status"][b] = n, ret, te, tr, status
        out["enc"][b] = o.encode()
        out["agent"][b], out["step_count"][b], out["carry"][b] = o.state[:3], o.state[3], o.carry
    out["streams"] = [r.bit_generator.state for r in rngs]
    return out


def continue_ref(first: dict, pi, model, max_steps, prob, **kw):
    """A second slip_rollout_ref call on the state and the streams the first one left."""
    return slip_rollout_ref(first["enc"], first["agent"], pi, model, max_steps, prob, carry=first["carry"],
                            step_count=first["step_count"], rngs=first["rngs"], **kw)


def stream_fields(streams) -> dict:
    """A list of numpy bit_generator.state dicts in the layout of MiniGridVecEnv.slip_streams()."""
    return {"state": np.array([s["state"]["state"] for s in streams], object),
            "inc": np.array([s["state"]["inc"] for s in streams], object),
            "has_uint32": np.array([s["has_uint32"] for s in streams], np.int64),
            "uinteger": np.array([s["uinteger"] for s in streams], np.int64)}


def fresh_streams(seed0: int, B: int, doubles=None) -> dict:
    """default_rng(seed0 + b) for every b, advanced by doubles[b] calls of random()."""
    rngs = [np.random.default_rng(seed0 + b) for b in range(B)]
    if doubles is not None:
        for r, k in zip(rngs, doubles):
            if k:
                r.random(int(k))
    return stream_fields([r.bit_generator.state for r in rngs])


def discounted_goal(res_steps, res_ret, res_terminated, gamma: float) -> np.ndarray:
    """g per env: gamma^(steps-1) if it ended on the goal (terminated with a positive return), else 0."""
    hit = np.asarray(res_terminated, bool) & (np.asarray(res_ret) > 0)
    return np.where(hit, gamma ** (np.asarray(res_steps, np.float64) - 1.0), 0.0)


def z_score(g: np.ndarray, v_start: float) -> tuple[float, float]:
    """(mean(g), (mean(g) - V*[start]) / (std(g, ddof=1) / sqrt(B)))."""
    g = np.asarray(g, np.float64)
    se = g.std(ddof=1) / np.sqrt(len(g))
    return float(g.mean()), float((g.mean() - v_start) / se)


_STAT: dict = {}


def stat_case(env_id: str, B: int = 4096, prob: float = 0.8, gamma: float = 0.9, seed0: int = 0) -> dict:
    """The Monte-Carlo check of the DP's slip model against the env (built once per process): B copies of
    the reset(seed=0) grid of env_id with max_steps B, pi* and V* of oracle.value_iteration(slip_p=prob)
    in fp64, and the restatement's rollout of pi* under set_slip(prob, seed0)."""
    key = (env_id, B, prob, gamma, seed0)
    if key in _STAT:
        return _STAT[key]
    from oracle import oracle

    enc1, agent1, env = rr.grids(env_id, 1)
    o = oracle.value_iteration(0, rr.cells_of(enc1), gamma=gamma, tol=1e-13, slip_p=prob, dtype="f64")
    enc, agent = np.repeat(enc1, B, axis=0), np.repeat(agent1, B, axis=0)
    pi = np.repeat(o["pi"], B, axis=0)
    v_start = float(o["V"][0, rr.start_states(enc1, agent1, "xyd")[0]])
    ref = slip_rollout_ref(enc, agent, pi, "xyd", B, prob, seed0, see_through=env.see_through_walls)
    c = {"env_id": env_id, "enc": enc, "agent": agent, "pi": pi, "max_steps": B, "prob": prob, "gamma": gamma,
         "seed0": seed0, "v_start": v_start, "ref": ref, "see_through": env.see_through_walls}
    _STAT[key] = c
    return c
