"""The argument rules of the Python front end (dp.ValueIteration, vector.MiniGridVecEnv), checked before any
device work: plain functions of the handle's numbers (B, S, A, horizon, N, ...) over numpy alone, so every refusal
is reachable without a GPU or the built library (tests/test_args_cpu.py).
"""
from __future__ import annotations

import numpy as np


# ---------------------------------------------------------------- policy arrays: int8 action lanes
def int8_lanes(pi, rows_of) -> tuple[np.ndarray, int]:
    """(contiguous int8 array, rows T) of an integer policy array.  Checked in this order: the dtype kind, the
    shape (`rows_of(shape)` returns T or raises the caller's own message), then that every entry fits int8."""
    a = np.asarray(pi)
    if a.dtype.kind not in "iu":
        raise ValueError(f"policy must be an integer array (int8 action lanes), got dtype {a.dtype}")
    T = rows_of(a.shape)
    if a.dtype != np.int8:
        if a.size and (a.min() < -128 or a.max() > 127):
            raise ValueError("policy entries do not fit int8 action lanes")
        a = a.astype(np.int8)
    return np.ascontiguousarray(a), T


def evaluate_policy(pi, B: int, S: int, horizon: int = 0, rows: bool = False) -> tuple[np.ndarray, int]:
    """evaluate / policy_iteration / is_optimal: (B, S); with `rows` on a finite horizon also (horizon, B, S)."""
    rows = rows and horizon > 0

    def rows_of(shape):
        if shape == (B, S):
            return 1
        if rows and shape == (horizon, B, S):
            return horizon
        want = f"{(B, S)}" + (f" or {(horizon, B, S)}" if rows else "")
        raise ValueError(f"policy of shape {shape} does not match the handle's {want}")

    return int8_lanes(pi, rows_of)


def occupancy_policy(pi, B: int, S: int, N: int) -> tuple[np.ndarray, int]:
    """occupancy: (B, S) or (N, B, S), row t applying at step_count t."""
    def rows_of(shape):
        if shape == (B, S):
            return 1
        if shape == (N, B, S):
            return N
        raise ValueError(f"policy of shape {shape} does not match {(B, S)} or {(N, B, S)}"
                         f" (rows T = {shape[0] if len(shape) == 3 else '?'})")

    return int8_lanes(pi, rows_of)


def rollout_policy(pi, B: int, S: int, model: str) -> tuple[np.ndarray, int]:
    """rollout / policy_actions: (B, S), or (T, B, S) with T > 1 (the row is step_count)."""
    def rows_of(shape):
        if shape == (B, S):
            return 1
        if len(shape) != 3 or shape[0] < 1 or shape[1:] != (B, S):
            raise ValueError(f"policy of shape {shape} is neither {(B, S)} nor (T, {B}, {S}) of the {model} model")
        return shape[0]

    a, T = int8_lanes(pi, rows_of)
    if a.ndim == 3 and T == 1:
        raise ValueError("a time-indexed policy needs T > 1 rows; pass (B, S) for a stationary one")
    return a, T


# ---------------------------------------------------------------- dp.ValueIteration
def max_iters(n) -> int:
    if int(n) <= 0:
        raise ValueError("max_iters must be > 0")
    return int(n)


def values_t_horizon(values_t, horizon: int) -> None:
    """evaluate_opts / evaluate_opts_device: every V_t is kept only on a finite horizon."""
    if values_t and horizon == 0:
        raise ValueError("values_t needs a finite horizon")


def evaluate_rows(T, values_t: bool, horizon: int) -> int:
    """evaluate_opts_device: the policy rows T (1 or the horizon), then values_t_horizon."""
    T = int(T)
    if T != 1 and not (horizon > 0 and T == horizon):
        raise ValueError(f"policy rows T = {T}: 1 or the handle's horizon ({horizon})")
    values_t_horizon(values_t, horizon)
    return T


def occupancy_steps(n_steps, horizon: int) -> int:
    """The N of a forward pass: the horizon on a finite-horizon handle, n_steps otherwise."""
    if horizon > 0:
        if n_steps is not None and int(n_steps) != horizon:
            raise ValueError(f"n_steps = {n_steps} on a finite-horizon handle: None or the horizon {horizon}")
        return horizon
    if n_steps is None:
        raise ValueError("n_steps is required on a horizon-0 handle")
    return int(n_steps)


def occupancy_start(start, B: int, S: int, np_dtype) -> tuple[np.ndarray | None, np.ndarray | None]:
    """(state indices int32 (B,), None) or (None, mu_0 (B, S) of the handle's dtype)."""
    st = np.asarray(start)
    if st.shape == (B,) and st.dtype.kind in "iu":
        return np.ascontiguousarray(np.clip(st.astype(np.int64), -1, 2 ** 31 - 1), np.int32), None
    if st.shape == (B, S):
        return None, np.ascontiguousarray(st, np_dtype)
    raise ValueError(f"start of shape {st.shape} is neither {(B,)} state indices nor a {(B, S)} array")


# ---------------------------------------------------------------- vector.MiniGridVecEnv
def rollout_budget(max_steps) -> int:
    """rollout's max_steps as the library takes it: 0 for None (no budget)."""
    n_max = 0 if max_steps is None else int(max_steps)
    if max_steps is not None and n_max <= 0:
        raise ValueError("max_steps must be > 0 (None: no budget)")
    return n_max


def trace_arrays(trace, full_len: int, cap: int, B: int):
    """(states int32 (n, B), actions int8 (n, B), n) for trace=True (n = full_len) or a number of steps,
    at most cap rows (0: no cap); (None, None, 0) for no trace."""
    if not trace:
        return None, None, 0
    n = full_len if trace is True else int(trace)
    if n <= 0:
        raise ValueError("trace must be True, False or a positive number of steps")
    n = min(n, cap) if cap else n
    return np.empty((n, B), np.int32), np.empty((n, B), np.int8), n


def seed_args(seed, mask, B: int):
    """(seed int, mask uint8 (B,) or None) of a seeding of one stream per env, slip or explore."""
    seed = int(seed)
    if not 0 <= seed <= 2**64 - B:
        raise ValueError(f"seed .. seed + {B} must fit 64 bits (one SeedSequence entropy int each)")
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask).reshape(B), np.uint8)
    return seed, mask


def slip_random_action(random_action) -> int:
    """set_slip's random_action as the library takes it: -1 for None (a uniform draw)."""
    ra = -1 if random_action is None else int(random_action)
    if random_action is not None and ra < 0:
        raise ValueError(f"random_action must be an env action 0..6 or None, got {random_action}")
    return ra


def q_n_act(n_act, A: int, model: str) -> int:
    n_act = A if n_act is None else int(n_act)
    if not 1 <= n_act <= A:
        raise ValueError(f"n_act must be in 1..{A} for the {model} model, got {n_act}")
    return n_act


def q_table(Q, B: int, S: int, A: int) -> np.ndarray:
    if Q is None:
        return np.zeros((B, S, A), np.float64)
    q = np.asarray(Q)
    if q.dtype != np.float64:
        raise ValueError(f"Q must be float64 (fp32 tables are out of scope), got dtype {q.dtype}")
    if q.shape != (B, S, A):
        raise ValueError(f"Q of shape {q.shape} is not {(B, S, A)}")
    return np.array(q, np.float64, order="C")  # the caller's table stays as it is


def q_params(n_steps, alpha, gamma, eps):
    n_steps = int(n_steps)
    if n_steps <= 0:
        raise ValueError(f"n_steps must be > 0, got {n_steps}")
    if n_steps >= 2**31:
        raise ValueError("n_steps must fit int32")
    alpha, gamma, eps = float(alpha), float(gamma), float(eps)
    if not 0.0 <= eps <= 1.0:  # NaN fails both
        raise ValueError(f"eps must be in [0, 1], got {eps}")
    if alpha != alpha or gamma != gamma:
        raise ValueError("alpha and gamma must not be NaN")
    return n_steps, alpha, gamma, eps
