"""Batched MiniGrid stepping on one GPU: B envs resident in HBM, one HIP launch per step.

The reference vectorises with gymnasium's in-process SyncVectorEnv (tests/test_envs.py:310-330),
which loops MiniGridEnv.step (minigrid_env.py:520-590) serially.  Here every env's grid planes and
agent state live in HBM and one envs_step_kernel launch advances all of them (csrc/envs.hip).
Grids are generated on the host by the reference-exact generators (envs.py) and uploaded on reset.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _args, _lib, gen
from .registry import make


@dataclass
class RolloutResult:
    """What MiniGridVecEnv.rollout collected, per env."""
    steps: np.ndarray       # (B,) int32 steps taken in this call
    ret: np.ndarray         # (B,) float64 their rewards, summed in step order (the env's own _reward / NoDeath cost)
    terminated: np.ndarray  # (B,) bool flags of the last step taken
    truncated: np.ndarray   # (B,) bool
    status: np.ndarray      # (B,) int32: 0, or the MGDP_E_* code that stopped the env (it was not stepped further)
    states: np.ndarray | None = None   # trace: (max steps, B) int32 state index before each step, -1 unused
    actions: np.ndarray | None = None  # trace: (max steps, B) int8 env action of each step, -1 unused

    @property
    def ok(self) -> bool:
        return bool((self.status == 0).all())


@dataclass
class QLearnResult:
    """What MiniGridVecEnv.q_learn did, per env."""
    Q: np.ndarray          # (B, S, A) float64 the table after the call (A: the model's lanes)
    steps: np.ndarray      # (B,) int32 steps taken in this call (n_steps, fewer only with a status)
    episodes: np.ndarray   # (B,) int32 episodes that ended (terminated or truncated) inside the call
    wins: np.ndarray       # (B,) int32 those that ended on the goal (terminated with a positive reward)
    ret: np.ndarray        # (B,) float64 the env's own rewards of every step, summed in step order
    status: np.ndarray     # (B,) int32: 0, or the MGDP_E_* code that kept / stopped the env
    states: np.ndarray | None = None   # trace: (n, B) int32 state index before each of the first n steps, -1 unused
    actions: np.ndarray | None = None  # trace: (n, B) int8 env action executed at each (after the slip), -1 unused

    @property
    def ok(self) -> bool:
        return bool((self.status == 0).all())


class MiniGridVecEnv:
    """B independent envs of one registered id (same W, H), stepped together on one GPU.

    step(actions) -> (obs, reward, terminated, truncated, info) with obs = {"image": (B,V,V,3) uint8,
    "direction": (B,) int32, "mission": [str]*B}.  autoreset=True resets finished envs right after
    the step with their next seed (the returned obs is then the reset observation and the final
    observation is in info["final_obs_image"]).
    """

    def __init__(self, env_id: str, num_envs: int, device: int = 0, autoreset: bool = False,
                 no_death_types: tuple = (), death_cost: float = -1.0, **kwargs):
        """no_death_types / death_cost: NoDeath(env, no_death_types, death_cost) applied inside the
        step kernel (wrappers.py:799-872)."""
        self.env_id = env_id
        self.num_envs = int(num_envs)
        self.autoreset = autoreset
        self._gen = make(env_id, **kwargs)  # host-side generator (one instance reused per seed)
        self._gpu_gen = gen.supported(self._gen)  # reset(seed) batches generated on the GPU
        self.device = device
        self.W, self.H = self._gen.width, self._gen.height
        self.view = self._gen.agent_view_size
        self.max_steps = self._gen.max_steps
        self.see_through = self._gen.see_through_walls
        self.mission = self._gen.mission
        self.L = _lib.load()
        _lib.require_gpu()
        h = ctypes.c_void_p()
        _lib.check(self.L.mgdp_envs_create(device, self.num_envs, self.W, self.H, self.view, ctypes.byref(h)),
                   "mgdp_envs_create")
        self.h = h
        if no_death_types:
            assert "goal" not in no_death_types, "goal cannot be a death cell"
            from .core import OBJECT_TO_IDX

            mask = 0
            for t in no_death_types:
                mask |= 1 << OBJECT_TO_IDX[t]
            _lib.check(self.L.mgdp_envs_set_nodeath(h, mask, float(death_cost)), "mgdp_envs_set_nodeath")
        B, V = self.num_envs, self.view
        self._obs = np.zeros((B, V, V, 3), np.uint8)
        self._dir = np.zeros(B, np.int32)
        self._rew = np.zeros(B, np.float64)
        self._term = np.zeros(B, np.uint8)
        self._trunc = np.zeros(B, np.uint8)
        self._status = np.zeros(B, np.int32)
        self._seeds = np.zeros(B, np.int64)
        self._next_seed = 0
        self._held = False  # Box contents planes in use (set_contents)
        self._ms_cap = self.max_steps  # the largest max_steps loaded: bounds a rollout's trace
        self._explore = False  # the explore streams of q_learn are seeded

    def close(self):
        if getattr(self, "h", None):
            self.L.mgdp_envs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- raw state upload
    def load(self, enc: np.ndarray, agent: np.ndarray, max_steps=None, see_through=None, mask=None, held=None):
        """Upload grids (B, W, H, 3) x-major encodings and agents (B, 3) = (x, y, dir).  held: what
        each Box cell holds (Box(contains=...)), the same layout, type 0 = nothing (set_contents)."""
        B = self.num_envs
        enc = np.ascontiguousarray(enc, np.uint8)
        agent = np.ascontiguousarray(agent, np.int32)
        assert enc.shape == (B, self.W, self.H, 3) and agent.shape == (B, 3)
        ms = np.full(B, self.max_steps if max_steps is None else 0, np.int32)
        if max_steps is not None:
            ms[:] = np.asarray(max_steps, np.int32)
        see = np.full(B, 1 if self.see_through else 0, np.uint8)
        if see_through is not None:
            see[:] = np.asarray(see_through, np.uint8)
        self._ms_cap = max(int(ms.max()), self._ms_cap if mask is not None else 0)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        _lib.check(self.L.mgdp_envs_load(self.h, _lib.ptr(enc), _lib.ptr(agent), _lib.ptr(ms), _lib.ptr(see),
                                         _lib.ptr(m)), "mgdp_envs_load")
        if held is not None:
            if mask is not None:  # the other envs keep theirs
                cur = self.get_contents()[0]
                sel = np.asarray(mask, bool)
                cur[sel] = np.asarray(held, np.uint8)[sel]
                held = cur
            self.set_contents(held)

    def set_contents(self, held=None, carry_held=None):
        """Box(contains=...) (world_object.py:272-294): held (B, W, H, 3) = the (type, colour, state)
        each Box cell holds, carry_held (B, 3) = what a carried Box holds (None = unchanged).  Toggling
        a Box then puts its object in the cell, and a carried Box keeps it (mgdp_envs_set_contents)."""
        B = self.num_envs
        h = None if held is None else np.ascontiguousarray(held, np.uint8)
        c = None if carry_held is None else np.ascontiguousarray(carry_held, np.int32)
        assert h is None or h.shape == (B, self.W, self.H, 3)
        assert c is None or c.shape == (B, 3)
        _lib.check(self.L.mgdp_envs_set_contents(self.h, _lib.ptr(h), _lib.ptr(c)), "mgdp_envs_set_contents")
        self._held = True

    def get_contents(self):
        """(held (B, W, H, 3), carry_held (B, 3)): what the Boxes hold now (zeros: nothing)."""
        B = self.num_envs
        held = np.zeros((B, self.W, self.H, 3), np.uint8)
        carry_held = np.zeros((B, 3), np.int32)
        _lib.check(self.L.mgdp_envs_get_contents(self.h, _lib.ptr(held), _lib.ptr(carry_held)),
                   "mgdp_envs_get_contents")
        return held, carry_held

    def _generate(self, seeds):
        seeds = np.asarray(seeds, np.int64)
        if self._gpu_gen and len(seeds) and (np.diff(seeds) == 1).all():
            # consecutive seeds: one generator launch (csrc/gen.hip) instead of a host loop
            out = gen.generate(self._gen, int(seeds[0]), len(seeds), device=self.device)
            return out["enc"], out["agent"]
        encs, agents = [], []
        for s in seeds:
            e, a = self._gen.generate(seed=int(s))
            encs.append(e)
            agents.append(a)
        return np.stack(encs), np.array(agents, np.int32)

    def observe(self):
        _lib.check(self.L.mgdp_envs_observe(self.h, _lib.ptr(self._obs), _lib.ptr(self._dir)), "mgdp_envs_observe")
        return self._obs_dict()

    def _obs_dict(self):
        return {"image": self._obs.copy(), "direction": self._dir.copy(), "mission": [self.mission] * self.num_envs}

    # ---------------------------------------------------------------- gym-style API
    def reset(self, seed: int | None = None):
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        self._seeds = np.arange(self.num_envs, dtype=np.int64) + int(seed)
        self._next_seed = int(seed) + self.num_envs
        enc, agent = self._generate(self._seeds)
        self.load(enc, agent)
        return self.observe(), {"seeds": self._seeds.copy()}

    def step(self, actions):
        a = np.ascontiguousarray(np.asarray(actions).reshape(self.num_envs), np.int32)
        rc = self.L.mgdp_envs_step(self.h, _lib.ptr(a), _lib.ptr(self._obs), _lib.ptr(self._dir),
                                   _lib.ptr(self._rew), _lib.ptr(self._term), _lib.ptr(self._trunc),
                                   _lib.ptr(self._status))
        if rc == _lib.MGDP_E_ACTION:
            bad = np.flatnonzero(self._status == _lib.MGDP_E_ACTION)
            raise ValueError(f"Unknown action: {actions[bad[0]] if len(bad) else actions} (env {bad.tolist()})")
        _lib.check(rc, "mgdp_envs_step")
        obs = self._obs_dict()
        term = self._term.astype(bool)
        trunc = self._trunc.astype(bool)
        info = {}
        if self.autoreset:
            done = term | trunc
            if done.any():
                info["final_obs_image"] = obs["image"].copy()
                idx = np.flatnonzero(done)
                seeds = self._next_seed + np.arange(len(idx))
                self._next_seed += len(idx)
                self._seeds[idx] = seeds
                enc = np.zeros((self.num_envs, self.W, self.H, 3), np.uint8)
                agent = np.zeros((self.num_envs, 3), np.int32)
                e, ag = self._generate(seeds)
                enc[idx], agent[idx] = e, ag
                mask = done.astype(np.uint8)
                self.load(enc, agent, mask=mask)
                obs = self.observe()
        return obs, self._rew.copy(), term, trunc, info

    def step_device(self, actions, obs, direction, reward, terminated, truncated, status):
        """Zero-copy step on device buffers (torch CUDA tensors or raw device pointers as ints),
        asynchronous on the handle's stream.  Raw pointers skip every per-call conversion."""
        p = _lib.ptr
        rc = self.L.mgdp_envs_step_device(self.h, p(actions), p(obs), p(direction), p(reward), p(terminated),
                                          p(truncated), p(status))
        if rc:
            _lib.check(rc, "mgdp_envs_step_device")

    # ---------------------------------------------------------------- tabular policies
    def _model_of(self, model, callers):
        """The model's name ("auto": the generator's) for the calls that run the envs as they are, refused
        where they cannot: autoreset, or Box contents on the handle."""
        from . import dp
        from .envs import DoorKeyEnv

        if self.autoreset:
            raise ValueError(f"{callers} run the envs as they are: not with autoreset=True")
        if self._held:
            raise ValueError("Box contents (set_contents) are in use: outside the XYD and DoorKey models")
        if model == "auto":
            model = "doorkey" if isinstance(self._gen, DoorKeyEnv) else "xyd"
        if model not in dp.MODELS:
            raise ValueError(f"unknown model {model!r}")
        return model

    def _policy_of(self, policy, model):
        """(pi int8 (T*B, S) contiguous, T, model id) of a (B, S) / (T, B, S) integer array or a VIResult,
        checked before any device work (_args.rollout_policy)."""
        from . import dp

        if isinstance(policy, dp.VIResult):
            if model == "auto":
                model = policy.model
            policy = policy.pi
        model = self._model_of(model, "rollout / policy_actions")
        pi, T = _args.rollout_policy(policy, self.num_envs, dp.n_states(model, self.W, self.H), model)
        return pi, T, dp.MODELS[model]

    def policy_actions(self, policy, model: str = "auto", return_status: bool = False):
        """(B,) int32: the env action `policy` takes at every env's current state (mgdp_envs_policy_actions),
        -1 where it has none (a lane outside the model's, a grid or carry outside the model, step_count
        beyond a time-indexed policy); return_status also gives the per-env status."""
        pi, T, mid = self._policy_of(policy, model)
        acts = np.zeros(self.num_envs, np.int32)
        status = np.zeros(self.num_envs, np.int32)
        _lib.check(self.L.mgdp_envs_policy_actions(self.h, mid, _lib.ptr(pi), T, _lib.ptr(acts), _lib.ptr(status)),
                   "mgdp_envs_policy_actions")
        return (acts, status) if return_status else acts

    def rollout(self, policy, model: str = "auto", max_steps: int | None = None,
                trace: bool | int = False) -> "RolloutResult":
        """Execute a tabular policy on every env from its current state, in one launch
        (mgdp_envs_rollout): until the env terminates, truncates or has taken max_steps steps (None:
        no budget).  policy: (B, S) int8 action lanes in ValueIteration.policy()'s order, (T, B, S) as
        policy_t() (the row is step_count), or a VIResult.  A per-env problem never raises: it is that
        env's status (see RolloutResult).  trace=True records states and actions of every step taken (up
        to the envs' max_steps rows of B entries each are allocated), trace=n those of the first n steps.
        A later call continues where this one stopped.  After set_slip() every step's action first passes
        the env's slip stream; the trace then holds the executed actions."""
        pi, T, mid = self._policy_of(policy, model)
        B = self.num_envs
        n_max = _args.rollout_budget(max_steps)
        steps, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
        ret = np.zeros(B, np.float64)
        term, trunc = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
        # no env outlives its max_steps from step_count 0; a budget bounds it further
        ts, ta, tlen = _args.trace_arrays(trace, max(int(self._ms_cap), 1), n_max, B)
        _lib.check(self.L.mgdp_envs_rollout(self.h, mid, _lib.ptr(pi), T, n_max, _lib.ptr(steps), _lib.ptr(ret),
                                            _lib.ptr(term), _lib.ptr(trunc), _lib.ptr(status), _lib.ptr(ts), _lib.ptr(ta),
                                            tlen), "mgdp_envs_rollout")
        if trace:
            k = min(int(steps.max(initial=0)), tlen)
            ts, ta = ts[:k].copy(), ta[:k].copy()
        return RolloutResult(steps, ret, term.astype(bool), trunc.astype(bool), status, ts, ta)

    def policy_actions_device(self, pi, T: int, model: str, actions, status):
        """policy_actions on device buffers (torch CUDA tensors or raw pointers), asynchronous on the
        handle's stream: pi int8 [T][B][S] (T = 1: [B][S]), actions / status int32 (B,)."""
        from . import dp

        p = _lib.ptr
        rc = self.L.mgdp_envs_policy_actions_device(self.h, dp.MODELS[model], p(pi), int(T), p(actions), p(status))
        if rc:
            _lib.check(rc, "mgdp_envs_policy_actions_device")

    def rollout_device(self, pi, T: int, model: str, max_steps, steps, ret, terminated, truncated, status,
                       trace_state=None, trace_action=None, trace_len: int = 0):
        """rollout on device buffers (torch CUDA tensors or raw pointers), asynchronous on the handle's
        stream: pi int8 [T][B][S], e.g. ValueIteration.device_buffers()[1] of a solved handle (no host
        copy); steps / status int32, ret float64, terminated / truncated uint8, all (B,); the trace
        int32 / int8 [trace_len][B] or None.  max_steps None or <= 0: no budget."""
        from . import dp

        if self.autoreset:
            raise ValueError("rollout runs the envs as they are: not with autoreset=True")
        p = _lib.ptr
        rc = self.L.mgdp_envs_rollout_device(self.h, dp.MODELS[model], p(pi), int(T), int(max_steps or 0), p(steps), p(ret),
                                             p(terminated), p(truncated), p(status), p(trace_state), p(trace_action),
                                             int(trace_len))
        if rc:
            _lib.check(rc, "mgdp_envs_rollout_device")

    # ---------------------------------------------------------------- slip
    def _read_streams(self, fn, name):
        """The records that `fn` (a stream table's getter) copies out, as slip_streams() documents them."""
        B = self.num_envs
        st = np.zeros((B, 4), np.uint64)
        half = np.zeros((B, 2), np.uint32)
        _lib.check(fn(self.h, _lib.ptr(st), _lib.ptr(half)), name)
        wide = st.astype(object)
        return {"state": (wide[:, 0] << 64) | wide[:, 1], "inc": (wide[:, 2] << 64) | wide[:, 3],
                "has_uint32": half[:, 0].astype(np.int64), "uinteger": half[:, 1].astype(np.int64)}

    def set_slip(self, prob: float = 0.9, seed: int = 0, random_action: int | None = None, mask=None):
        """StochasticActionWrapper(env, prob, random_action) (wrappers.py:775-796) with one stream per env:
        env b draws from numpy.random.default_rng(seed + b).  From now on every step of rollout() keeps
        the policy's action with probability prob and otherwise executes random_action, or a uniform
        draw of the env actions 0..5 (None).  mask (B,): reseed only those envs' streams (prob and
        random_action always hold for the whole handle); the first call must seed them all.  step(),
        policy_actions(), load() and reset() neither draw nor touch the streams (mgdp_envs_set_slip)."""
        seed, m = _args.seed_args(seed, mask, self.num_envs)
        ra = _args.slip_random_action(random_action)
        _lib.check(self.L.mgdp_envs_set_slip(self.h, float(prob), ra, seed, _lib.ptr(m)), "mgdp_envs_set_slip")

    def clear_slip(self):
        """Back to the plain rollout; a later set_slip seeds every stream anew."""
        _lib.check(self.L.mgdp_envs_clear_slip(self.h), "mgdp_envs_clear_slip")

    def slip_streams(self):
        """The envs' streams as numpy's Generator.bit_generator.state holds them, one array of B entries per
        field: {"state", "inc"}: Python ints (128 bits, object arrays), "has_uint32", "uinteger": the
        buffered half-word.  Synchronises."""
        return self._read_streams(self.L.mgdp_envs_get_slip_streams, "mgdp_envs_get_slip_streams")

    def slip_actions(self, actions):
        """(B,) int32: one slip decision per env on `actions` (mgdp_envs_slip_actions) -- what the slip
        rollout does between the policy lookup and the step.  A negative action (policy_actions' "none")
        passes through without a draw."""
        a = np.ascontiguousarray(np.asarray(actions).reshape(self.num_envs), np.int32)
        out = np.zeros(self.num_envs, np.int32)
        _lib.check(self.L.mgdp_envs_slip_actions(self.h, _lib.ptr(a), _lib.ptr(out)), "mgdp_envs_slip_actions")
        return out

    def slip_actions_device(self, actions, out):
        """slip_actions on device buffers (torch CUDA tensors or raw pointers), int32 (B,), asynchronous on
        the handle's stream; out may be actions itself."""
        rc = self.L.mgdp_envs_slip_actions_device(self.h, _lib.ptr(actions), _lib.ptr(out))
        if rc:
            _lib.check(rc, "mgdp_envs_slip_actions_device")

    # ---------------------------------------------------------------- tabular Q-learning
    def _q_model(self, model, n_act):
        """(model name, model id, S, A, n_act) checked before any device work."""
        from . import dp

        model = self._model_of(model, "q_learn / q_greedy")
        S, A = dp.n_states(model, self.W, self.H), dp.n_actions(model)
        return model, dp.MODELS[model], S, A, _args.q_n_act(n_act, A, model)

    def set_explore(self, seed: int = 0, mask=None):
        """Seed the explore streams of q_learn: env b draws from numpy.random.default_rng(seed + b).  mask
        (B,): reseed only those envs; the first call must seed them all.  Independent of the slip streams."""
        seed, m = _args.seed_args(seed, mask, self.num_envs)
        _lib.check(self.L.mgdp_envs_set_explore(self.h, seed, _lib.ptr(m)), "mgdp_envs_set_explore")
        self._explore = True

    def explore_streams(self):
        """The explore streams in the layout of slip_streams().  Synchronises."""
        return self._read_streams(self.L.mgdp_envs_get_explore_streams, "mgdp_envs_get_explore_streams")

    def q_learn(self, n_steps: int, Q=None, model: str = "auto", alpha: float = 0.5, gamma: float = 0.99,
                eps: float = 0.1, n_act: int | None = None, unit_goal: bool = False, seed: int | None = None,
                trace: bool | int = False) -> "QLearnResult":
        """Tabular Q-learning of every env on its own table, n_steps eps-greedy steps through step() in one
        launch (mgdp_envs_q_learn).  Q: (B, S, A) float64 in the model's state and lane order (None: zeros;
        it is copied, the result holds the new table).  Each step: u = rng.random(); u < eps draws a lane of
        the first n_act uniformly, else the lowest-index argmax of Q[b][s][:n_act]; then
        Q[s][lane] += alpha * (target - Q[s][lane]) with target = r, or r + gamma * max Q[s'][:n_act] unless
        the step terminated (unit_goal: a positive r counts as 1).  An episode that terminates or truncates
        restarts from the env's state at the call; the call leaves every env exactly as it found it.
        seed: env b explores with numpy.random.default_rng(seed + b); None continues the streams (seeded
        with 0 at the first use).  After set_slip() the executed action passes the env's slip stream, the
        update stays on the chosen lane.  A per-env problem is that env's status, never an exception.
        trace=True records state and executed action of every step, trace=n of the first n."""
        model, mid, S, A, n_act = self._q_model(model, n_act)
        n_steps, alpha, gamma, eps = _args.q_params(n_steps, alpha, gamma, eps)
        B = self.num_envs
        q = _args.q_table(Q, B, S, A)
        ts, ta, tlen = _args.trace_arrays(trace, n_steps, n_steps, B)
        if seed is not None:
            self.set_explore(seed)
        elif not self._explore:
            self.set_explore(0)
        steps, episodes, wins, status = (np.zeros(B, np.int32) for _ in range(4))
        ret = np.zeros(B, np.float64)
        p = _lib.ptr
        _lib.check(self.L.mgdp_envs_q_learn(self.h, mid, p(q), n_steps, alpha, gamma, eps, n_act, int(bool(unit_goal)),
                                            p(steps), p(episodes), p(wins), p(ret), p(status), p(ts), p(ta), tlen),
                   "mgdp_envs_q_learn")
        return QLearnResult(q, steps, episodes, wins, ret, status, ts, ta)

    def q_learn_device(self, Q, n_steps: int, model: str, steps, episodes, wins, ret, status, alpha: float = 0.5,
                       gamma: float = 0.99, eps: float = 0.1, n_act: int | None = None, unit_goal: bool = False,
                       trace_state=None, trace_action=None, trace_len: int = 0):
        """q_learn on device buffers (torch CUDA tensors or raw pointers), asynchronous on the handle's
        stream: Q float64 [B][S][A] updated in place; steps / episodes / wins / status int32, ret float64, all
        (B,); the trace int32 / int8 [trace_len][B] or None.  The explore streams must have been seeded
        (set_explore, or an earlier q_learn)."""
        model, mid, S, A, n_act = self._q_model(model, n_act)
        n_steps, alpha, gamma, eps = _args.q_params(n_steps, alpha, gamma, eps)
        p = _lib.ptr
        rc = self.L.mgdp_envs_q_learn_device(self.h, mid, p(Q), n_steps, alpha, gamma, eps, n_act, int(bool(unit_goal)),
                                             p(steps), p(episodes), p(wins), p(ret), p(status), p(trace_state),
                                             p(trace_action), int(trace_len))
        if rc:
            _lib.check(rc, "mgdp_envs_q_learn_device")

    def q_greedy(self, Q, model: str = "auto", n_act: int | None = None, values: bool = False):
        """(B, S) int8: the lowest-index argmax of Q[b][s][:n_act] for every (b, s) (mgdp_envs_q_greedy) -- a
        policy for rollout() and ValueIteration.evaluate(); values=True also returns that maximum, (B, S)
        float64."""
        model, mid, S, A, n_act = self._q_model(model, n_act)
        if Q is None:
            raise ValueError("q_greedy needs a table")
        B = self.num_envs
        q = _args.q_table(Q, B, S, A)
        pi = np.zeros((B, S), np.int8)
        vq = np.zeros((B, S), np.float64) if values else None
        _lib.check(self.L.mgdp_envs_q_greedy(self.h, mid, _lib.ptr(q), n_act, _lib.ptr(pi), _lib.ptr(vq)),
                   "mgdp_envs_q_greedy")
        return (pi, vq) if values else pi

    def q_greedy_device(self, Q, model: str, pi, values=None, n_act: int | None = None):
        """q_greedy on device buffers, asynchronous on the handle's stream: Q float64 [B][S][A], pi int8
        [B][S], values float64 [B][S] or None."""
        model, mid, S, A, n_act = self._q_model(model, n_act)
        rc = self.L.mgdp_envs_q_greedy_device(self.h, mid, _lib.ptr(Q), n_act, _lib.ptr(pi), _lib.ptr(values))
        if rc:
            _lib.check(rc, "mgdp_envs_q_greedy_device")

    def enable_timing(self, on: bool):
        """Time every step-kernel launch with a HIP event pair on the launch itself."""
        _lib.check(self.L.mgdp_envs_enable_timing(self.h, int(on)), "mgdp_envs_enable_timing")

    def kernel_time(self):
        """(total ms, launches) of the step kernel since enable_timing(True); synchronises."""
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        _lib.check(self.L.mgdp_envs_kernel_time(self.h, ctypes.byref(ms), ctypes.byref(n)), "mgdp_envs_kernel_time")
        return ms.value, n.value

    def set_stream(self, stream):
        _lib.check(self.L.mgdp_envs_set_stream(self.h, ctypes.c_void_p(int(stream) if stream else 0)),
                   "mgdp_envs_set_stream")

    def get_state(self):
        B = self.num_envs
        enc = np.zeros((B, self.W, self.H, 3), np.uint8)
        agent = np.zeros((B, 3), np.int32)
        carry = np.zeros((B, 2), np.int32)
        sc = np.zeros(B, np.int32)
        _lib.check(self.L.mgdp_envs_get_state(self.h, _lib.ptr(enc), _lib.ptr(agent), _lib.ptr(carry), _lib.ptr(sc)),
                   "mgdp_envs_get_state")
        st = {"enc": enc, "agent": agent, "carry": carry, "step_count": sc}
        if self._held:
            st["held"], st["carry_held"] = self.get_contents()
        return st
