"""numpy restatement of policy evaluation under the handle options, in the
pattern of tests/policy_ref.py: the transition tables are the oracle's (orc_build_table, or
orc_xyd_next_nodeath for NoDeath lava), the loops are plain numpy in the working type T in the
operation order of orc_vi_ex (oracle/mgdp_oracle.c, DEFINE_VI_EX):

    R_t = T(_reward(t+1, H)) where the table has done and R == 1 (finite horizon), else T(R)
    Qd  = where(done, R_t, R_t + g*V[s'])
    Vn  = Qd[pi_t]                                           deterministic
    Vn  = p*Qd[pi_t] + c*(((((Q0+Q1)+Q2)+Q3)+Q4)+Q5)         slip, c = T((1-p)/6)
    Vn[absorbing] = 0

NoDeath with horizon 0 is PolicyRef's evaluate / improve / policy_iteration on the NoDeath tables.
A finite horizon is the backward induction V_H = 0, t = H-1 .. 0, exactly H sweeps, every V_t kept.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from minigrid_dynamicprogramming_amd.core import OBJECT_TO_IDX
from oracle import oracle
from tests.policy_ref import PolicyRef


@functools.lru_cache(maxsize=None)
def _nodeath_table_cached(key: bytes, W: int, H: int, death_cost: float):
    cells = np.frombuffer(key, np.uint8).reshape(H, W)
    L = oracle.lib()
    S, A = W * H * 4, 7
    nxt = np.full((S, A), -1, np.int32)
    rew = np.zeros((S, A), np.float64)
    done = np.zeros((S, A), np.uint8)
    sp, dn, r = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
    cp = cells.ctypes.data_as(ctypes.c_void_p)
    psp, pr, pdn = ctypes.addressof(sp), ctypes.addressof(r), ctypes.addressof(dn)
    for s in range(S):
        for a in range(A):
            if L.orc_xyd_next_nodeath(cp, W, H, s, a, float(death_cost), psp, pr, pdn):
                nxt[s, a], rew[s, a], done[s, a] = sp.value, r.value, dn.value
    return nxt, rew, done


def nodeath_table(cells: np.ndarray, death_cost: float):
    """nxt, rew, done (S x 7) of one XYD grid under NoDeath lava: orc_xyd_next_nodeath state by state,
    as orc_vi_ex builds its table with lava_mode = 1 (absorbing: nxt -1, rew 0, done 0)."""
    cells = np.ascontiguousarray(cells, np.uint8)
    H, W = cells.shape
    return _nodeath_table_cached(cells.tobytes(), W, H, float(death_cost))


def lava_entries(ref, cells, W, first=0):
    """Per env: the steps n >= first of a reference rollout trace (tests/rollout_ref.py, trace_len covering
    the episode) that moved forward into a lava cell."""
    lava = OBJECT_TO_IDX["lava"]
    off = (1, W, -1, -W)
    B = cells.shape[0]
    m = np.zeros(B, np.int64)
    for b in range(B):
        flat = cells[b].reshape(-1)
        for n in range(first, int(ref["steps"][b])):
            s, a = int(ref["states"][n, b]), int(ref["actions"][n, b])
            if a == 2 and flat[(s >> 2) + off[s & 3]] == lava:
                m[b] += 1
    return m


class PolicyOptsRef(PolicyRef):
    def __init__(self, model: int, cells: np.ndarray, gamma=0.99, tol=1e-6, slip_p=None, dtype="f32",
                 lava="terminal", death_cost=-1.0, horizon=0):
        cells = np.ascontiguousarray(cells, np.uint8)
        if cells.ndim == 2:
            cells = cells[None]
        self.B = cells.shape[0]
        self.T = np.float32 if dtype == "f32" else np.float64
        if lava == "nodeath":
            assert model == 0, "NoDeath lava is defined for the XYD model"
            tabs = [nodeath_table(cells[b], death_cost) for b in range(self.B)]
        else:
            tabs = [oracle.build_table(model, cells[b]) for b in range(self.B)]
        nxt = np.stack([t[0] for t in tabs]).astype(np.int64)          # (B, S, A)
        self.S, self.A = nxt.shape[1:]
        self.absorb = nxt[:, :, 0] < 0                                  # (B, S)
        self.idx = np.where(nxt < 0, 0, nxt)
        r64 = np.stack([t[1] for t in tabs])
        self.R = r64.astype(self.T)
        self.done = np.stack([t[2] for t in tabs]).astype(bool)
        self.goal = self.done & (r64 == 1.0)                            # where the horizon's R_t applies
        self.g = self.T(gamma)
        self.tol = float(tol)
        self.slip = slip_p is not None
        if self.slip:
            assert model == 0, "slip is defined for the XYD model"
            self.p = self.T(slip_p)
            self.c = self.T((1.0 - float(slip_p)) / 6.0)
        self.rows = np.arange(self.B)[:, None, None]
        self.H = int(horizon)

    def check_rows(self, pi):
        """pi as (T, B, S) int8 rows, T = 1 or H.  ValueError for any other T, and for a lane outside
        [0, A) on a valid state: the lowest offending grid, its largest offending t, that row's lowest
        offending state."""
        pi = np.asarray(pi).astype(np.int8)
        rows = pi.reshape(1, self.B, self.S) if pi.ndim == 2 else pi
        T = rows.shape[0]
        if T != 1 and not (self.H > 0 and T == self.H):
            raise ValueError(f"policy rows T = {T}")
        if rows.shape[1:] != (self.B, self.S):
            raise ValueError(f"policy of shape {pi.shape}")
        bad = ~self.absorb[None] & ((rows < 0) | (rows >= self.A))
        if bad.any():
            b = int(np.nonzero(bad.any(axis=(0, 2)))[0][0])
            t = int(np.nonzero(bad[:, b].any(axis=1))[0][-1])
            s = int(np.nonzero(bad[t, b])[0][0])
            raise ValueError(f"policy: grid {b} t {t} state {s}: action {rows[t, b, s]} is outside [0, {self.A})")
        return rows

    def evaluate_horizon(self, pi):
        """Backward induction of a stationary (B, S) or time-indexed (H, B, S) policy: V (= V_0), Vt
        (H, B, S), pi (the normalised pi_0), sweeps H, dv = max|V_0 - V_1|, grid_sweeps all H."""
        assert self.H > 0
        rows = self.check_rows(pi)
        H, T = self.H, rows.shape[0]
        V = np.zeros((self.B, self.S), self.T)
        Vt = np.empty((H, self.B, self.S), self.T)
        dv = 0.0
        for t in range(H - 1, -1, -1):
            rg = self.T(oracle.reward(t + 1, H))
            R = np.where(self.goal, rg, self.R)
            Q = np.where(self.done, R, R + self.g * V[self.rows, self.idx])
            lanes = np.clip(rows[t if T > 1 else 0], 0, self.A - 1).astype(np.int64)
            Qa = np.take_along_axis(Q, lanes[..., None], axis=2)[..., 0]
            Vn = self.p * Qa + self.c * self._s6(Q) if self.slip else Qa
            Vn = Vn.astype(self.T)
            Vn[self.absorb] = 0
            dv = float(np.abs(Vn - V).max())
            V = Vn
            Vt[t] = V
        pi0 = rows[0].copy()
        pi0[self.absorb] = -1
        return {"V": V, "Vt": Vt, "pi": pi0, "sweeps": H, "dv": dv, "converged": True,
                "grid_sweeps": np.full(self.B, H, np.int32)}
