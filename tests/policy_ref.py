"""numpy restatement of policy evaluation, greedy improvement and policy iteration (DESIGN.md
section 13), in the style of oracle/numpy_vi.py: the transition tables are the oracle's pinned
orc_build_table, the loops are plain numpy in the working type T, in the operation order of the kernels:

    Q  = where(done, R, R + g*V[s'])
    Vn = Q[pi]                                               deterministic
    Vn = p*Q[pi] + c*(((((Q0+Q1)+Q2)+Q3)+Q4)+Q5)             slip, c = T((1-p)/6)
    Vn[absorbing] = 0;  dv = max|Vn - V|;  stop after the sweep with dv < tol, or at max_sweeps
    improve: Qs = Q (deterministic) or p*Q + c*s6;  pi' = pi where Qs[pi] == max(Qs), else argmax(Qs)

TEST INFRASTRUCTURE ONLY: the literal global loop the GPU result must equal bit for bit, plus the
per-grid executed sweeps of the fixed-point-completion protocol (mgdp_vi_get_grid_sweeps).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle


class PolicyRef:
    def __init__(self, model: int, cells: np.ndarray, gamma=0.99, tol=1e-6, slip_p=None, dtype="f32"):
        cells = np.ascontiguousarray(cells, np.uint8)
        if cells.ndim == 2:
            cells = cells[None]
        self.B = cells.shape[0]
        self.T = np.float32 if dtype == "f32" else np.float64
        tabs = [oracle.build_table(model, cells[b]) for b in range(self.B)]
        nxt = np.stack([t[0] for t in tabs]).astype(np.int64)          # (B, S, A)
        self.S, self.A = nxt.shape[1:]
        self.absorb = nxt[:, :, 0] < 0                                  # (B, S)
        self.idx = np.where(nxt < 0, 0, nxt)
        self.R = np.stack([t[1] for t in tabs]).astype(self.T)
        self.done = np.stack([t[2] for t in tabs]).astype(bool)
        self.g = self.T(gamma)
        self.tol = float(tol)
        self.slip = slip_p is not None
        if self.slip:
            assert model == 0, "slip is defined for the XYD model"
            self.p = self.T(slip_p)
            self.c = self.T((1.0 - float(slip_p)) / 6.0)
        self.rows = np.arange(self.B)[:, None, None]

    # Q of every (grid, state, action) on V (B, S), deterministic form
    def q(self, V):
        return np.where(self.done, self.R, self.R + self.g * V[self.rows, self.idx])

    def _s6(self, Q):
        return ((((Q[..., 0] + Q[..., 1]) + Q[..., 2]) + Q[..., 3]) + Q[..., 4]) + Q[..., 5]

    def normalise(self, pi):
        """The policy as the handle stores it (absorbing states -1); ValueError on a lane outside
        [0, A) of a valid state."""
        pi = np.asarray(pi).astype(np.int8).reshape(self.B, self.S).copy()
        bad = ~self.absorb & ((pi < 0) | (pi >= self.A))
        if bad.any():
            b, s = np.argwhere(bad)[0]
            raise ValueError(f"policy: grid {b} state {s}: action {pi[b, s]} is outside [0, {self.A})")
        pi[self.absorb] = -1
        return pi

    def sweep(self, V, pi):
        """One evaluation sweep: (V_{k+1}, per-grid max|dV|)."""
        Q = self.q(V)
        Qa = np.take_along_axis(Q, np.clip(pi, 0, self.A - 1).astype(np.int64)[..., None], axis=2)[..., 0]
        Vn = self.p * Qa + self.c * self._s6(Q) if self.slip else Qa
        Vn = Vn.astype(self.T)
        Vn[self.absorb] = 0
        return Vn, np.abs(Vn - V).max(axis=1).astype(np.float64)

    def evaluate(self, pi, max_sweeps=10000):
        """The literal global loop from V_0 = 0.  grid_sweeps: what each grid executes under the
        protocol -- its own stop k_e; the grids that stopped with dV != 0 go on to K0 = max k_e; a
        fallback sweep past K0 is executed by the grids whose last dV != 0 only."""
        pi = self.normalise(pi)
        V = np.zeros((self.B, self.S), self.T)
        dvs = []
        k = 0
        while True:
            k += 1
            V, dve = self.sweep(V, pi)
            dvs.append(dve)
            dv = float(dve.max())
            if dv < self.tol or k >= max_sweeps:
                break
        dvs = np.stack(dvs)                                   # (K, B)
        own = np.empty(self.B, np.int64)
        for e in range(self.B):
            hit = np.nonzero(dvs[:, e] < self.tol)[0]
            own[e] = hit[0] + 1 if len(hit) else k
        K0 = int(own.max())
        gs = own.copy()
        last = dvs[own - 1, np.arange(self.B)]
        go = (own < K0) & (last != 0)
        gs[go] = K0
        last[go] = dvs[K0 - 1, go]
        for j in range(K0 + 1, k + 1):
            go = last != 0
            gs[go] = j
            last[go] = dvs[j - 1, go]
        return {"V": V, "pi": pi, "sweeps": k, "dv": dv, "converged": dv < self.tol,
                "grid_sweeps": gs.astype(np.int32)}

    def improve(self, V, pi):
        """(pi', changed): argmax of Q on V, lowest index among ties, the current action kept when it
        attains the maximum; absorbing states -1 and never counted."""
        pi = np.asarray(pi).astype(np.int8).reshape(self.B, self.S)
        Q = self.q(V)
        Qs = (self.p * Q + (self.c * self._s6(Q))[..., None]).astype(self.T) if self.slip else Q
        best = Qs.max(axis=2)
        arg = Qs.argmax(axis=2).astype(np.int8)
        inr = (pi >= 0) & (pi < self.A)
        qc = np.take_along_axis(Qs, np.clip(pi, 0, self.A - 1).astype(np.int64)[..., None], axis=2)[..., 0]
        new = np.where(inr & (qc == best), pi, arg).astype(np.int8)
        new[self.absorb] = -1
        return new, int(((new != pi) & ~self.absorb).sum())

    def policy_iteration(self, pi0=None, max_iters=1000, max_sweeps=10000):
        pi = np.full((self.B, self.S), 2, np.int8) if pi0 is None else np.asarray(pi0)
        changes, total, it = [], 0, 0
        while True:
            ev = self.evaluate(pi, max_sweeps)
            pi, ch = self.improve(ev["V"], ev["pi"])
            changes.append(ch)
            total += ev["sweeps"]
            it += 1
            if ch == 0 or it >= max_iters:
                break
        return {"V": ev["V"], "pi": pi, "iters": it, "eval_sweeps": total, "changes": changes, "changed": ch,
                "dv": ev["dv"], "sweeps": ev["sweeps"], "grid_sweeps": ev["grid_sweeps"]}
