"""numpy restatement of the depth form of a deterministic XYD solve from V_0 = 0 (csrc/vi_serve_depth.h,
DESIGN.md section 20), for the tests: the breadth-first depth of every state from the goal, the table
g(1) = 1, g(n + 1) = fl(gamma * g(n)) in the working type, and from them K, dV_K, V_{K-1} and V_K without
sweeping.  The state graph comes from the oracle's transition table (orc_build_table), not from the
kernel's row masks, so this is a second statement of the search, not a copy of it."""
import numpy as np

from oracle import oracle


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


def depths(cells):
    """(S,) int64: d(s) >= 1, or 0 where no depth exists.  d = 1: a valid state with an action that ends the
    episode with reward 1 (its front cell is the goal); a state's successors are its non-terminal moves."""
    nxt, rew, done = oracle.build_table(0, np.ascontiguousarray(cells, np.uint8))
    S = nxt.shape[0]
    valid = nxt[:, 0] >= 0
    d = np.zeros(S, np.int64)
    d[valid & ((done != 0) & (rew == 1.0)).any(axis=1)] = 1
    move = valid[:, None] & (done == 0)
    succ = np.where(move, nxt, 0)
    level = 1
    while (d == level).any():
        reach = ((d[succ] > 0) & move).any(axis=1)
        level += 1
        d[valid & reach & (d == 0)] = level
    return d


def g_table(gamma, dtype, n):
    """g[0] = 0 (no depth), g[1] = 1, g[k + 1] = fl(gamma * g[k]) in the working type."""
    T = np_type(dtype)
    g = np.zeros(n + 1, T)
    if n >= 1:
        g[1] = 1
    for k in range(1, n):
        g[k + 1] = T(gamma) * g[k]
    return g


def closed_form(cells, gamma=0.99, tol=1e-6, max_sweeps=10000, dtype="f64"):
    """{"D", "sweeps" (K), "dv" (dV_K), "V" (V_K), "Vprev" (V_{K-1})}: V_k[s] = g(d(s)) if d(s) <= k else 0,
    dV_k = g(k) if some state has depth k else 0, K = min(first k with dV_k < tol, max_sweeps)."""
    d = depths(cells)
    D = int(d.max())
    K = None
    v = np_type(dtype)(1)
    for k in range(1, min(D, max_sweeps) + 1):  # g(k) on the fly: the table need not reach max_sweeps
        if float(v) < tol:
            K = k
            break
        v = np_type(dtype)(gamma) * v
    if K is None:
        K = D + 1 if tol > 0 else max_sweeps
    K = min(K, max_sweeps)
    g = g_table(gamma, dtype, max(min(K, D), 1))
    dv = float(g[K]) if K <= D else 0.0

    def V_at(k):
        return np.where((d > 0) & (d <= k), g[np.minimum(d, len(g) - 1)], 0).astype(np_type(dtype))

    return {"D": D, "sweeps": K, "dv": dv, "V": V_at(K)[None], "Vprev": V_at(K - 1)[None]}


def last_sweep(cells, Vprev, gamma, dtype):
    """One Jacobi sweep on V_{K-1} (the oracle's arithmetic, numpy_vi's): (V_K, pi_K)."""
    T = np_type(dtype)
    nxt, rew, done = oracle.build_table(0, np.ascontiguousarray(cells, np.uint8))
    absorb = nxt[:, 0] < 0
    V = np.asarray(Vprev, T).reshape(-1)
    R = rew.astype(T)
    Q = np.where(done != 0, R, R + T(gamma) * V[np.where(nxt < 0, 0, nxt)])
    Vn = Q.max(axis=1)
    Vn[absorb] = 0
    pi = Q.argmax(axis=1).astype(np.int8)
    pi[absorb] = -1
    return Vn[None], pi[None]
