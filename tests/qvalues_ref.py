"""numpy restatement of the action-value read-out on tests/policy_ref.PolicyRef and
tests/policy_opts_ref.PolicyOptsRef (the NoDeath tables): the table whose argmax PolicyRef.improve takes.

    Q   = ref.q(V)                                          where(done, R, R + g*V[s'])
    Q   = (p*Q + (c*s6)[..., None]).astype(T)               slip, s6 = ((((Q0+Q1)+Q2)+Q3)+Q4)+Q5
    Q[absorbing] = 0
    opt = bit a set iff Q[s, a] == max_a' Q[s, a'];  0 on absorbing states

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

from tests.policy_opts_ref import PolicyOptsRef
from tests.policy_ref import PolicyRef


def make_ref(model: int, cells, gamma=0.99, tol=1e-6, slip_p=None, dtype="f32", lava="terminal", death_cost=-1.0):
    if lava == "nodeath":
        return PolicyOptsRef(model, cells, gamma, tol, slip_p, dtype, lava=lava, death_cost=death_cost)
    return PolicyRef(model, cells, gamma, tol, slip_p, dtype)


def q_table(ref: PolicyRef, V) -> np.ndarray:
    """(B, S, A) in ref.T."""
    V = np.asarray(V, ref.T).reshape(ref.B, ref.S)
    Q = ref.q(V)
    if ref.slip:
        Q = (ref.p * Q + (ref.c * ref._s6(Q))[..., None]).astype(ref.T)
    Q = np.array(Q, ref.T)
    Q[ref.absorb] = 0
    return Q


def opt_sets(ref: PolicyRef, Q) -> np.ndarray:
    """(B, S) uint8."""
    hit = Q == Q.max(-1, keepdims=True)
    opt = (hit.astype(np.uint32) << np.arange(ref.A, dtype=np.uint32)).sum(-1).astype(np.uint8)
    opt[ref.absorb] = 0
    return opt


def q_and_opt(ref: PolicyRef, V):
    Q = q_table(ref, V)
    return Q, opt_sets(ref, Q)


def lowest_bit(opt) -> np.ndarray:
    """(B, S) int8: the lowest set bit of each entry, -1 where none is set."""
    o = np.asarray(opt).astype(np.int64)
    low = np.full(o.shape, -1, np.int8)
    for a in range(7, -1, -1):
        low[(o >> a) & 1 == 1] = a
    return low


def lane_bit(opt, pi) -> np.ndarray:
    """(B, S) bool: whether pi's lane has its bit in opt (False for a lane outside [0, 8))."""
    lane = np.asarray(pi).astype(np.int64)
    inr = (lane >= 0) & (lane < 8)
    return (((np.asarray(opt).astype(np.int64) >> np.where(inr, lane, 0)) & 1) == 1) & inr
