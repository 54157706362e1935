"""Tabular value iteration over Minigrid grids on MI355X (front end of csrc/vi.hip).

The reference has no DP code; this module implements the build-defined
value iteration of DESIGN.md "A9", whose transition is the reference MiniGridEnv.step
(minigrid/minigrid_env.py:520-583).  Models:
  "xyd"      s = (y*W + x)*4 + dir, 7 actions (Empty, FourRooms, LavaCrossing, SimpleCrossing)
  "doorkey"  s = (((y*W + x)*4 + dir)*2 + has_key)*2 + door_open, 5 action lanes
             (left, right, forward, pickup, toggle)
Optional slip transitions follow StochasticActionWrapper (minigrid/wrappers.py:775-796).
All arithmetic runs in libmgdp.so on the GPU; results are bit-identical to the CPU oracle.
"""
from __future__ import annotations

import atexit
import ctypes
import hashlib
import weakref
from dataclasses import dataclass

import numpy as np

from . import _args, _lib
from . import checkpoint as _ckpt
from .core import COLOR_TO_IDX, OBJECT_TO_IDX

MODELS = {"xyd": _lib.MODEL_XYD, "doorkey": _lib.MODEL_DOORKEY}
DTYPES = {"f32": _lib.F32, "f64": _lib.F64}
METHODS = {"fused": _lib.METHOD_FUSED, "sweep": _lib.METHOD_SWEEP}
MAPPINGS = {"cell": _lib.MAP_CELL, "sa": _lib.MAP_SA}
DOORKEY_ACTIONS = (0, 1, 2, 3, 5)  # DP action lane -> env action (doorkey.py:25-33)


def n_states(model: str, W: int, H: int) -> int:
    return W * H * (4 if model == "xyd" else 16)


def n_actions(model: str) -> int:
    return 7 if model == "xyd" else 5


def state_index(model: str, W: int, x: int, y: int, d: int, has_key: int = 0, door_open: int = 0) -> int:
    s = (y * W + x) * 4 + d
    if model == "doorkey":
        s = (s * 2 + has_key) * 2 + door_open
    return s


def to_cells(grids) -> tuple[np.ndarray, np.ndarray | None]:
    """Normalise grids to (B, H, W) OBJECT_TO_IDX cell codes (+ the (B, W, H, 3) encodings when known).

    Accepts: env objects with .grid, Grid objects (or lists of either), (B, W, H, 3) encodings in
    the reference's x-major Grid.encode() layout, or cell codes (H, W) / (B, H, W)."""
    if isinstance(grids, np.ndarray):
        a = grids
        if a.ndim == 4:  # (B, W, H, 3) encodings
            enc = np.ascontiguousarray(a, dtype=np.uint8)
            return np.ascontiguousarray(enc[..., 0].transpose(0, 2, 1)), enc
        if a.ndim == 2:  # (H, W) cells
            a = a[None]
        if a.ndim != 3:
            raise ValueError("expected (B, W, H, 3) encodings or (B, H, W) / (H, W) cell codes")
        return np.ascontiguousarray(a, dtype=np.uint8), None
    if hasattr(grids, "grid") or hasattr(grids, "encode"):
        grids = [grids]
    encs = []
    for g in grids:
        grid = g.grid if hasattr(g, "grid") else g
        encs.append(grid.encode())
    enc = np.ascontiguousarray(np.stack(encs), dtype=np.uint8)
    return np.ascontiguousarray(enc[..., 0].transpose(0, 2, 1)), enc


def infer_model(cells: np.ndarray) -> str:
    has_door = (cells == OBJECT_TO_IDX["door"]).any()
    has_key = (cells == OBJECT_TO_IDX["key"]).any()
    return "doorkey" if (has_door or has_key) else "xyd"


def check_doorkey_encoding(enc: np.ndarray):
    """DoorKey model preconditions that need colours/states: one LOCKED door, key of its colour."""
    for b in range(enc.shape[0]):
        t = enc[b, :, :, 0]
        door = np.argwhere(t == OBJECT_TO_IDX["door"])
        key = np.argwhere(t == OBJECT_TO_IDX["key"])
        if len(door) != 1 or len(key) != 1:
            raise ValueError(f"grid {b}: the DoorKey model needs exactly one door and one key")
        dx, dy = door[0]
        kx, ky = key[0]
        if enc[b, dx, dy, 2] != 2:
            raise ValueError(f"grid {b}: the DoorKey model starts from a locked door")
        if enc[b, dx, dy, 1] != enc[b, kx, ky, 1]:
            raise ValueError(f"grid {b}: key colour does not match the door")


@dataclass
class VIResult:
    V: np.ndarray        # (B, S) float32 / float64
    pi: np.ndarray       # (B, S) int8 action lane (-1 = absorbing)
    sweeps: int
    converged: bool
    dv: float            # max |V_k - V_{k-1}| at the last sweep
    model: str
    W: int
    H: int
    # policy_iteration() only: improvement iterations, their evaluation sweeps summed, and the states the
    # last improvement changed (0: the policy is stable); `sweeps` is then the last evaluation's count
    iters: int | None = None
    eval_sweeps: int | None = None
    changed: int | None = None

    def value(self, b: int, x: int, y: int, d: int, has_key: int = 0, door_open: int = 0):
        return self.V[b, state_index(self.model, self.W, x, y, d, has_key, door_open)]

    def action(self, b: int, x: int, y: int, d: int, has_key: int = 0, door_open: int = 0) -> int:
        """Greedy env action (Actions id) at a state."""
        lane = int(self.pi[b, state_index(self.model, self.W, x, y, d, has_key, door_open)])
        if lane < 0:
            return -1
        return DOORKEY_ACTIONS[lane] if self.model == "doorkey" else lane


@dataclass
class OccupancyResult:
    """The forward pass of a policy (ValueIteration.occupancy).  Planes are (B, S) in
    the handle's dtype, +0 on walls; the derived arrays are (B,) float64 sums over masks taken from the cells
    (None when the cells were installed from device memory)."""
    mu: np.ndarray              # mu_N on valid states; on goal / terminal-lava states the mass absorbed there
    occ: np.ndarray             # sum_t disc[t] * mu_t: the discounted visitation (d^pi up to normalisation)
    ret: np.ndarray             # the discounted reward collected on entering goal (and NoDeath lava) states
    mu_t: np.ndarray | None     # (N, B, S) every mu_t, with every_step=True
    n_steps: int
    model: str
    W: int
    H: int
    p_goal: np.ndarray | None = None           # mass on goal cells after N steps
    p_lava: np.ndarray | None = None           # mass on lava cells (absorbed; under lava="nodeath" standing there)
    p_alive: np.ndarray | None = None          # mass still on empty / floor cells
    expected_return: np.ndarray | None = None  # sum of ret = <mu_0, V_0^pi>
    expected_steps: np.ndarray | None = None   # sum of occ: the expected number of steps taken (for gamma = 1)


@dataclass
class ActionValues:
    """The action values of a value function (dp.action_values)."""
    Q: np.ndarray        # (B, S, A) in the handle's dtype, +0 on walls and absorbing states
    opt: np.ndarray      # (B, S) uint8, bit a: Q[s, a] is the state's maximum; 0 on walls and absorbing states
    V: np.ndarray        # (B, S) the value function Q was read from (V*, or V^pi of the given policy)
    pi: np.ndarray       # (B, S) int8: pi*, or the evaluated policy (-1 = absorbing)
    sweeps: int
    model: str

    def advantage(self) -> np.ndarray:
        """Q - V[..., None] on valid states, +0 elsewhere."""
        valid = (self.opt != 0)[..., None]
        return np.where(valid, self.Q - self.V[..., None], self.Q.dtype.type(0))


def occupancy_masks(cells: np.ndarray) -> dict:
    """(B, S) masks of the XYD states standing on goal, lava and empty / floor cells of (B, H, W) cell codes."""
    flat = np.asarray(cells).reshape(cells.shape[0], -1)
    goal, lava = flat == OBJECT_TO_IDX["goal"], flat == OBJECT_TO_IDX["lava"]
    free = (flat == OBJECT_TO_IDX["empty"]) | (flat == OBJECT_TO_IDX["floor"])
    return {k: np.repeat(m, 4, axis=1) for k, m in (("goal", goal), ("lava", lava), ("alive", free))}


def occupancy_derived(cells: np.ndarray, mu: np.ndarray, occ: np.ndarray, ret: np.ndarray) -> dict:
    """p_goal, p_lava, p_alive, expected_return, expected_steps per grid: float64 sums of the planes."""
    m = occupancy_masks(cells)
    B = mu.shape[0]

    def total(plane, mask=None):
        return np.array([np.sum(plane[b] if mask is None else plane[b][mask[b]], dtype=np.float64) for b in range(B)])

    return {"p_goal": total(mu, m["goal"]), "p_lava": total(mu, m["lava"]), "p_alive": total(mu, m["alive"]),
            "expected_return": total(ret), "expected_steps": total(occ)}


# Handles still open at interpreter exit are destroyed explicitly: a lone-grid handle may keep a
# persistent solver resident on its stream, and destroy() asks it to leave and drains the stream.
_LIVE: "weakref.WeakSet[ValueIteration]" = weakref.WeakSet()


@atexit.register
def _close_live_handles():
    for vi in list(_LIVE):
        try:
            vi.close()
        except Exception:
            pass


class ValueIteration:
    """A batch of B grids resident on one GPU (an mgdp_vi handle); solve() may be called repeatedly.

    method "fused": one workgroup per grid, V in LDS for the whole solve (default; fastest).
    method "sweep": one launch per Jacobi sweep, V double-buffered in HBM.
    mapping "cell": one thread per cell; "sa": one thread per (state, action) + wave max-reduce.
    """

    def __init__(self, grids, model: str = "auto", gamma: float = 0.99, tol: float = 1e-6,
                 slip_p: float | None = None, max_sweeps: int = 10000, dtype: str = "f32",
                 method: str = "fused", mapping: str = "cell", device: int = 0, stream=None,
                 lava: str = "terminal", death_cost: float = -1.0, horizon: int = 0,
                 keep_policy_t: bool = False):
        """lava="nodeath": NoDeath(no_death_types=("lava",), death_cost) semantics
        (wrappers.py:799-872).  horizon=H > 0: finite-horizon DP over step_count with the exact
        _reward() (minigrid_env.py:235-240), H = the env's max_steps; keep_policy_t keeps pi_t.
        Either option needs W*H <= 1024 (one thread per cell in one workgroup): ValueError above."""
        cells, enc = to_cells(grids)
        if model == "auto":
            model = infer_model(cells)
        if model not in MODELS:
            raise ValueError(f"unknown model {model!r}")
        if model == "doorkey" and enc is not None:
            check_doorkey_encoding(enc)
        self.L = _lib.load()
        _lib.require_gpu()
        B, H, W = cells.shape
        self.model, self.B, self.W, self.H = model, B, W, H
        self.S = n_states(model, W, H)
        self.dtype = dtype
        self.np_dtype = np.float32 if dtype == "f32" else np.float64
        self.tol = float(tol)
        self.max_sweeps = int(max_sweeps)
        d = _lib.ViDesc()
        d.model = MODELS[model]
        d.dtype = DTYPES[dtype]
        d.method = METHODS[method]
        d.mapping = MAPPINGS[mapping]
        d.B, d.W, d.H = B, W, H
        d.max_sweeps = self.max_sweeps
        d.device = device
        d.gamma = float(gamma)
        d.tol = float(tol)
        d.slip_p = -1.0 if slip_p is None else float(slip_p)
        if lava not in ("terminal", "nodeath"):
            raise ValueError(f"lava must be 'terminal' or 'nodeath', got {lava!r}")
        d.lava_mode = 1 if lava == "nodeath" else 0
        d.death_cost = float(death_cost)
        d.horizon = int(horizon)
        d.flags = 1 if keep_policy_t else 0
        self.horizon = int(horizon)
        self.method, self.lava = method, lava
        self.desc = d
        self._solve_args = None
        self._live = None  # the last solve()'s ctypes outputs while they are the current result
        self._sharded_args = None
        self._load_dev_fn = None
        h = ctypes.c_void_p()
        _lib.check(self.L.mgdp_vi_create(ctypes.byref(d), ctypes.byref(h)), "mgdp_vi_create")
        self.h = h
        _LIVE.add(self)
        if stream is not None:
            _lib.check(self.L.mgdp_vi_set_stream(h, _lib.dev_ptr(stream)), "mgdp_vi_set_stream")
        self.load(cells)

    @property
    def persistent(self) -> bool:
        """Whether solve() is served by the resident vi_serve_kernel (lone grid, fused, cell)."""
        on = ctypes.c_int32(0)
        _lib.check(self.L.mgdp_vi_persistent(self.h, ctypes.byref(on)), "mgdp_vi_persistent")
        return bool(on.value)

    @property
    def kernel_name(self) -> str:
        """The kernel kernel_time() times on this handle, as rocprofv3 lists it."""
        n = self.L.mgdp_vi_kernel_name(self.h)
        if n is None:
            _lib.check(_lib.MGDP_E_INVALID, "mgdp_vi_kernel_name")
        return n.decode()

    @property
    def variant(self) -> str:
        """Which loop of that kernel runs (mgdp_vi_variant): e.g. serve_ew, wave2, dk_rows, dk_half."""
        n = self.L.mgdp_vi_variant(self.h)
        if n is None:
            _lib.check(_lib.MGDP_E_INVALID, "mgdp_vi_variant")
        return n.decode()

    def load(self, grids):
        """Install new grids of the same shape (mgdp_vi_load_cells); the next solve uses them."""
        cells, enc = to_cells(grids)
        if cells.shape != (self.B, self.H, self.W):
            raise ValueError(f"grids of shape {cells.shape} do not match the handle's {(self.B, self.H, self.W)}")
        if self.model == "doorkey" and enc is not None:
            check_doorkey_encoding(enc)
        cells = np.ascontiguousarray(cells, np.uint8)
        _lib.check(self.L.mgdp_vi_load_cells(self.h, _lib.ptr(cells)), "mgdp_vi_load_cells")
        self._cells_digest = hashlib.sha256(cells.tobytes()).hexdigest()  # checkpoint() / resume()
        self._cells = cells  # occupancy(): the masks of its derived sums
        self.sweeps = 0
        self.converged = False
        self.dv = float("nan")

    def load_device(self, cells_ptr: int):
        """Install new grids from device memory (mgdp_vi_load_cells_device): B*H*W row-major type
        codes at `cells_ptr` (e.g. a torch uint8 tensor's data_ptr()), complete before the call and
        unchanged until the next solve returns.  A resident lone-grid server takes the grid with
        its next request, so this makes no HIP call; the bytes are not validated here."""
        if self._load_dev_fn is None:
            self._load_dev_fn = _lib.raw_fn("mgdp_vi_load_cells_device")
        rc = self._load_dev_fn(self.h, _lib.dev_ptr(cells_ptr))
        if rc:
            _lib.check(rc, "mgdp_vi_load_cells_device")
        self._cells_digest = None  # not read back: a checkpoint of these grids cannot be verified
        self._cells = None
        self.sweeps = 0
        self.converged = False
        self.dv = float("nan")

    def close(self):
        if getattr(self, "h", None):
            self.L.mgdp_vi_destroy(self.h)
            self.h = None
            self._solve_args = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- single-device solve
    def solve(self, last: bool = False) -> int:
        """Whole solve (mgdp_vi_solve).  last=True (mgdp_vi_solve_last): a resident lone-grid server
        leaves right after this solve instead of idling out; the next solve relaunches it."""
        if self._solve_args is None:  # reused ctypes arguments: nothing converted or allocated per solve
            self._out = (ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_int32(0))
            self._solve_args = (ctypes.c_void_p(self.h.value if isinstance(self.h, ctypes.c_void_p) else self.h),) + \
                tuple(ctypes.byref(o) for o in self._out)
            # a resident lone-grid server answers in ~10 us: keep the GIL across that call
            quick = self.persistent
            self._solve_fn = _lib.raw_fn("mgdp_vi_solve", keep_gil=quick)
            self._solve_last_fn = _lib.raw_fn("mgdp_vi_solve_last", keep_gil=quick)
        rc = (self._solve_last_fn if last else self._solve_fn)(*self._solve_args)
        if rc:
            _lib.check(rc, "mgdp_vi_solve")
        # the result stays in the ctypes outputs (sweeps / dv / converged read them): a served solve
        # takes a few microseconds, and converting and storing three attributes per call was a
        # measurable part of the host's turnaround between requests
        self._live = self._out
        return self._out[0].value

    # -- policy evaluation / improvement / policy iteration (DESIGN.md sections 13 and 19)
    def _call_result(self, name: str, *args) -> int:
        """`name`(handle, *args, &sweeps, &dv, &converged): the three become the handle's result."""
        k, dv, conv = ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_int32(0)
        _lib.check(getattr(self.L, name)(self.h, *args, ctypes.byref(k), ctypes.byref(dv), ctypes.byref(conv)), name)
        self.sweeps, self.dv, self.converged = k.value, dv.value, bool(conv.value)
        return self.sweeps

    def _call_policy_iteration(self, name: str, pi0, max_iters) -> dict:
        a = None if pi0 is None else _args.evaluate_policy(pi0, self.B, self.S)[0]
        max_iters = _args.max_iters(max_iters)
        it, tot, ch, dv = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0)
        _lib.check(getattr(self.L, name)(self.h, None if a is None else _lib.ptr(a), max_iters, ctypes.byref(it),
                                         ctypes.byref(tot), ctypes.byref(ch), ctypes.byref(dv)), name)
        # converged of the last evaluation: dv < tol unless max_sweeps capped it
        self.dv = dv.value
        self.converged = dv.value < self.tol
        # the last evaluation's K is the largest per-grid count (a grid below K ended at a fixed point)
        self.sweeps = int(self.grid_sweeps().max())
        return {"iters": it.value, "eval_sweeps": tot.value, "changed": ch.value, "dv": dv.value}

    def evaluate(self, pi) -> int:
        """V^pi of a policy (mgdp_vi_evaluate): pi is (B, S) int8 in policy()'s state order and action
        lanes; entries of absorbing states are ignored (stored as -1), an entry outside [0, A) on a
        valid state raises ValueError naming grid and state.  Returns the sweeps of the global
        stopping rule; values(), policy(), grid_sweeps() and result() then describe the evaluation.
        run_to / sweep / resume need a reset() afterwards; solve() works as before."""
        a, _ = _args.evaluate_policy(pi, self.B, self.S)
        return self._call_result("mgdp_vi_evaluate", _lib.ptr(a))

    def evaluate_device(self, pi_ptr: int | None = None) -> int:
        """evaluate() of a policy in device memory (mgdp_vi_evaluate_device): B*S int8 at `pi_ptr`
        (16-byte aligned, e.g. a torch int8 tensor's data_ptr()); None evaluates the handle's own pi
        buffer -- pi* right after a solve()."""
        return self._call_result("mgdp_vi_evaluate_device", _lib.dev_ptr(pi_ptr))

    def improve(self) -> int:
        """Greedy improvement on the handle's V (mgdp_vi_improve): pi(s) <- argmax_a Q(s, a), lowest
        index among ties except that the current action stays when it attains the maximum.  Returns
        the number of states whose action changed, over the batch."""
        n = ctypes.c_int64(0)
        _lib.check(self.L.mgdp_vi_improve(self.h, ctypes.byref(n)), "mgdp_vi_improve")
        return n.value

    def policy_iteration(self, pi0=None, max_iters: int = 1000) -> dict:
        """Policy iteration (mgdp_vi_policy_iteration) from pi0 ((B, S) int8; None: "forward" on every
        valid state): evaluate from V_0 = 0, improve, until no state changes or max_iters.  Returns
        dict(iters, eval_sweeps, changed, dv); values() is the last evaluation's V, policy() the final pi."""
        return self._call_policy_iteration("mgdp_vi_policy_iteration", pi0, max_iters)

    # -- the same under horizon / lava="nodeath" 
    def evaluate_opts(self, pi, values_t: bool = False) -> int:
        """evaluate() on any handle (mgdp_vi_evaluate_opts).  lava="nodeath", horizon 0: the discounted
        V^pi on the NoDeath tables.  horizon H > 0: backward induction, exactly H sweeps, of a stationary
        (B, S) or time-indexed (H, B, S) policy (policy_t()'s layout, the row is step_count before the
        step); values() is then V_0, policy() the normalised pi_0, and with values_t=True values_t()
        returns every V_t as (H, B, S).  A lane outside [0, A) on a valid state, in any row, raises
        ValueError naming grid, t and state.  On a plain handle: exactly evaluate().  Returns the sweeps."""
        a, T = _args.evaluate_policy(pi, self.B, self.S, self.horizon, rows=True)
        _args.values_t_horizon(values_t, self.horizon)
        vt = np.empty((self.horizon, self.B, self.S), self.np_dtype) if values_t else None
        self._values_t = None
        k = self._call_result("mgdp_vi_evaluate_opts", _lib.ptr(a), T, None if vt is None else _lib.ptr(vt))
        self._values_t = vt
        return k

    def values_t(self) -> np.ndarray:
        """(H, B, S): every V_t of the last evaluate_opts(pi, values_t=True)."""
        vt = getattr(self, "_values_t", None)
        if vt is None:
            raise ValueError("no V_t: call evaluate_opts(pi, values_t=True) on a finite-horizon handle first")
        return vt

    def evaluate_opts_device(self, pi_ptr: int | None = None, T: int = 1, values_t_ptr: int | None = None) -> int:
        """evaluate_opts() with the policy (T*B*S int8, T = 1 or the horizon) and optionally V_t (H*B*S of
        the handle's dtype) in device memory, 16-byte aligned (mgdp_vi_evaluate_opts_device).  pi_ptr None:
        the handle's own pi (T = 1) or pi_t (T = horizon, needs keep_policy_t) -- pi_t* right after solve()."""
        T = _args.evaluate_rows(T, values_t_ptr is not None, self.horizon)
        self._values_t = None
        return self._call_result("mgdp_vi_evaluate_opts_device", _lib.dev_ptr(pi_ptr), T, _lib.dev_ptr(values_t_ptr))

    def improve_opts(self) -> int:
        """improve() on a plain or lava="nodeath" handle (mgdp_vi_improve_opts); refused on a finite horizon."""
        n = ctypes.c_int64(0)
        _lib.check(self.L.mgdp_vi_improve_opts(self.h, ctypes.byref(n)), "mgdp_vi_improve_opts")
        return n.value

    def policy_iteration_opts(self, pi0=None, max_iters: int = 1000) -> dict:
        """policy_iteration() on a plain or lava="nodeath" handle (mgdp_vi_policy_iteration_opts); refused
        on a finite horizon (its greedy step is the solve itself)."""
        return self._call_policy_iteration("mgdp_vi_policy_iteration_opts", pi0, max_iters)

    # -- the forward pass of a policy
    def occupancy(self, pi, start, n_steps: int | None = None, every_step: bool = False) -> OccupancyResult:
        """The forward pass mu_{t+1} = P_pi^T mu_t of a policy (mgdp_vi_occupancy): exactly N steps, N the
        horizon on a finite-horizon handle and n_steps otherwise.  pi is (B, S) or (N, B, S) int8 lanes (row t
        applies at step_count t: policy_t()'s and rollout()'s layout); start is (B,) state indices (one-hot)
        or a (B, S) distribution mu_0.  XYD handles of W*H <= 1024 under any options; it reads the cells and
        the options only, so it works before solve() and changes nothing a later solve() sees.  ValueError:
        a lane outside [0, 7) on a valid state (naming grid, the smallest such t, and state), a start index out
        of range or on a wall / goal / terminal lava, mu_0 mass on one of those, rows other than 1 or N, a
        DoorKey handle.  every_step=True also returns every mu_t as (N, B, S)."""
        N = _args.occupancy_steps(n_steps, self.horizon)
        a, T = _args.occupancy_policy(pi, self.B, self.S, N)
        s_idx, mu0 = _args.occupancy_start(start, self.B, self.S, self.np_dtype)
        mu, occ, ret = (np.empty((self.B, self.S), self.np_dtype) for _ in range(3))
        mu_t = np.empty((N, self.B, self.S), self.np_dtype) if every_step else None
        _lib.check(self.L.mgdp_vi_occupancy(self.h, _lib.ptr(a), T, _lib.ptr(s_idx), _lib.ptr(mu0), N, _lib.ptr(mu),
                                            _lib.ptr(occ), _lib.ptr(ret), _lib.ptr(mu_t)), "mgdp_vi_occupancy")
        cells = getattr(self, "_cells", None)
        derived = occupancy_derived(cells, mu, occ, ret) if cells is not None else {}
        return OccupancyResult(mu, occ, ret, mu_t, N, self.model, self.W, self.H, **derived)

    def occupancy_device(self, pi_ptr: int, T: int, mu_ptr: int, start_ptr: int | None = None, mu0_ptr: int | None = None,
                         n_steps: int | None = None, occ_ptr: int | None = None, ret_ptr: int | None = None,
                         mu_t_ptr: int | None = None) -> int:
        """occupancy() on device memory (mgdp_vi_occupancy_device), on the handle's stream: the policy (T*B*S
        int8, T = 1 or N), start (B int32) or mu0 (B*S), and the outputs mu (required), occ, ret (B*S) and
        mu_t (N*B*S) of the handle's dtype, 16-byte aligned (start: 4).  Returns N; the results are complete."""
        N = _args.occupancy_steps(n_steps, self.horizon)
        p = _lib.dev_ptr
        _lib.check(self.L.mgdp_vi_occupancy_device(self.h, p(pi_ptr), int(T), p(start_ptr), p(mu0_ptr), N, p(mu_ptr),
                                                   p(occ_ptr), p(ret_ptr), p(mu_t_ptr)), "mgdp_vi_occupancy_device")
        return N

    # -- action values of the handle's V
    def action_values(self, optimal: bool = False):
        """Q(s, a) of the handle's current V (mgdp_vi_action_values): (B, S, A) in the handle's dtype -- Q* after
        solve(), Q^pi after evaluate(pi) -- bit for bit the values improve() compares; +0 on walls and absorbing
        states.  A = n_actions(model): XYD 7 (lanes 3..6 hold the same bits), DoorKey 5; the layout is
        MiniGridVecEnv.q_learn's, so an fp64 handle's table passes to q_learn(Q=...), q_greedy and rollout as it
        is.  optimal=True returns (Q, opt), opt as optimal_actions().  The handles improve_opts() admits; ValueError
        on a finite horizon and before any solve or evaluation.  Nothing of the handle changes."""
        Q = np.empty((self.B, self.S, n_actions(self.model)), self.np_dtype)
        opt = np.empty((self.B, self.S), np.uint8) if optimal else None
        _lib.check(self.L.mgdp_vi_action_values(self.h, _lib.ptr(Q), _lib.ptr(opt)), "mgdp_vi_action_values")
        return (Q, opt) if optimal else Q

    def optimal_actions(self) -> np.ndarray:
        """(B, S) uint8: bit a is set iff Q(s, a) equals max_a' Q(s, a') in the handle's dtype; 0 on walls and
        absorbing states.  The opt-only launch: no Q is allocated or written."""
        opt = np.empty((self.B, self.S), np.uint8)
        _lib.check(self.L.mgdp_vi_action_values(self.h, None, _lib.ptr(opt)), "mgdp_vi_action_values")
        return opt

    def action_values_device(self, q_ptr: int | None, opt_ptr: int | None = None) -> None:
        """action_values() into device memory (mgdp_vi_action_values_device), on the handle's stream: Q (B*S*A of
        the handle's dtype) at q_ptr and / or opt (B*S uint8) at opt_ptr, 16-byte aligned (e.g. torch tensors'
        data_ptr()); either may be None, not both.  The results are complete when it returns."""
        p = _lib.dev_ptr
        _lib.check(self.L.mgdp_vi_action_values_device(self.h, p(q_ptr), p(opt_ptr)), "mgdp_vi_action_values_device")

    def is_optimal(self, pi) -> np.ndarray:
        """(B, S) bool: whether pi's lane is a maximising action of the handle's V, whichever it chose among ties;
        True on walls and absorbing states (whatever their entry), False where a valid state's lane is outside
        [0, A).  pi as evaluate() takes it."""
        a, _ = _args.evaluate_policy(pi, self.B, self.S)
        opt = self.optimal_actions()
        lane = a.astype(np.int64)
        inr = (lane >= 0) & (lane < n_actions(self.model))
        hit = ((opt.astype(np.int64) >> np.where(inr, lane, 0)) & 1).astype(bool) & inr
        return hit | (opt == 0)

    # sweeps / dv / converged of the last result: read from solve()'s outputs while they are current
    def _result_attr(self, i, name):
        live = self.__dict__.get("_live")
        if live is not None:
            return (live[0].value, live[1].value, bool(live[2].value))[i]
        return self.__dict__[name]

    def _set_result_attr(self, name, v):
        live = self.__dict__.get("_live")
        if live is not None:  # leaving the live outputs: the other two keep their values
            self.__dict__.update(_sweeps=live[0].value, _dv=live[1].value, _converged=bool(live[2].value))
            self.__dict__["_live"] = None
        self.__dict__[name] = v

    sweeps = property(lambda self: self._result_attr(0, "_sweeps"), lambda self, v: self._set_result_attr("_sweeps", v))
    dv = property(lambda self: self._result_attr(1, "_dv"), lambda self, v: self._set_result_attr("_dv", v))
    converged = property(lambda self: self._result_attr(2, "_converged"),
                         lambda self, v: self._set_result_attr("_converged", v))

    def solve_sharded(self, comm) -> int:
        """One sharded solve with the library's own collectives (mgdp_vi_solve_sharded on a
        distributed.LibComm): every rank of the communicator calls it (or joins host-driven)."""
        if self._sharded_args is None or self._sharded_args[1] != comm.handle:
            self._sh_out = (ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_int32(0))
            self._sharded_args = (self.h, comm.handle) + tuple(ctypes.byref(o) for o in self._sh_out)
        _lib.check(self.L.mgdp_vi_solve_sharded(*self._sharded_args), "mgdp_vi_solve_sharded")
        k, dv, conv = self._sh_out
        self.sweeps, self.dv, self.converged = k.value, dv.value, bool(conv.value)
        return self.sweeps

    @property
    def sharded_capable(self) -> bool:
        """Whether mgdp_vi_solve_sharded runs this handle (fused method, no horizon / lava options)."""
        return self.method == "fused" and self.horizon == 0 and self.lava == "terminal"

    # -- multi-device protocol pieces (see distributed.py)
    def reset(self):
        _lib.check(self.L.mgdp_vi_reset(self.h), "mgdp_vi_reset")

    def run_local(self) -> int:
        k = ctypes.c_int32(0)
        _lib.check(self.L.mgdp_vi_run_local(self.h, ctypes.byref(k)), "mgdp_vi_run_local")
        return k.value

    def local_result(self) -> tuple[int, float]:
        """(max sweeps, max |dV| of each grid's last sweep) of the last launch (mgdp_vi_local_result):
        after run_local, dV of every grid at its own stopping sweep."""
        k = ctypes.c_int32(0)
        dv = ctypes.c_double(0)
        _lib.check(self.L.mgdp_vi_local_result(self.h, ctypes.byref(k), ctypes.byref(dv), None),
                   "mgdp_vi_local_result")
        return k.value, dv.value

    def run_to(self, k: int) -> float:
        dv = ctypes.c_double(0)
        _lib.check(self.L.mgdp_vi_run_to(self.h, int(k), ctypes.byref(dv)), "mgdp_vi_run_to")
        return dv.value

    def sweep(self) -> float:
        dv = ctypes.c_double(0)
        _lib.check(self.L.mgdp_vi_sweep(self.h, ctypes.byref(dv)), "mgdp_vi_sweep")
        return dv.value

    # -- the same protocol with device-resident K / dV (distributed.py over RCCL): enqueue only
    @property
    def protocol_device(self):
        """The torch device whose int64 buffers the *_dev steps read and write (None when this handle
        runs the host protocol only: sweep method, horizon or NoDeath options)."""
        if self.desc.method != _lib.METHOD_FUSED or self.horizon > 0 or self.desc.lava_mode != 0:
            return None
        dev = getattr(self, "_protocol_dev", None)
        if dev is None:
            import torch

            dev = self._protocol_dev = torch.device("cuda", self.desc.device)
        return dev

    def bind_stream(self, stream_ptr: int):
        """Launch on this hipStream_t from now on (no-op when it already does)."""
        if getattr(self, "_bound_stream", None) != int(stream_ptr):
            _lib.check(self.L.mgdp_vi_set_stream(self.h, _lib.dev_ptr(stream_ptr)), "mgdp_vi_set_stream")
            self._bound_stream = int(stream_ptr)

    def run_local_dev(self, pub):
        """pub: int64 CUDA tensor (or pointer) of 4 words <- {k max, dV bits, k min, 0}."""
        if getattr(self, "_rld_fn", None) is None:
            self._rld_fn = _lib.raw_fn("mgdp_vi_run_local_dev")
        rc = self._rld_fn(self.h, _lib.ptr(pub))
        if rc:
            _lib.check(rc, "mgdp_vi_run_local_dev")

    def run_to_dev(self, k, pub):
        """Every grid to exactly the sweep held by the int64 device word k; results into pub."""
        _lib.check(self.L.mgdp_vi_run_to_dev(self.h, _lib.ptr(k), _lib.ptr(pub)), "mgdp_vi_run_to_dev")

    def run_to_dev_sync(self, kdv) -> tuple[int, float, float]:
        """Every grid to exactly K = kdv[0] (int64 device words, read on the device), then wait on
        the host-mapped result: (K, this shard's dV at K, kdv[1] as a double)."""
        if getattr(self, "_sync_fn", None) is None:
            self._sync_fn = _lib.raw_fn("mgdp_vi_run_to_dev_sync")
            self._sync_out = (ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_double(0))
        k, dv, rule = self._sync_out
        rc = self._sync_fn(self.h, ctypes.c_void_p(kdv.data_ptr()), ctypes.byref(k), ctypes.byref(dv),
                           ctypes.byref(rule))
        if rc:
            _lib.check(rc, "mgdp_vi_run_to_dev_sync")
        return k.value, dv.value, rule.value

    def set_result(self, k: int, dv: float):
        _lib.check(self.L.mgdp_vi_set_result(self.h, int(k), float(dv)), "mgdp_vi_set_result")

    def finish(self, sweeps: int, dv: float):
        _lib.check(self.L.mgdp_vi_finish(self.h, int(sweeps)), "mgdp_vi_finish")
        self.sweeps, self.dv = int(sweeps), float(dv)
        self.converged = dv < self.tol

    # -- results
    def policy_t(self) -> np.ndarray:
        """Finite horizon with keep_policy_t: (H, B, S) int8, pi_t[t] = the greedy lane at step_count t."""
        out = np.empty((self.horizon, self.B, self.S), np.int8)
        _lib.check(self.L.mgdp_vi_get_policy_t(self.h, _lib.ptr(out)), "mgdp_vi_get_policy_t")
        return out

    def grid_sweeps(self) -> np.ndarray:
        """(B,) int32: the sweeps each grid executed (mgdp_vi_get_grid_sweeps) -- its own stopping
        sweep if it ended at an exact fixed point (complete for the global K), else K."""
        k = np.empty(self.B, np.int32)
        _lib.check(self.L.mgdp_vi_get_grid_sweeps(self.h, _lib.ptr(k)), "mgdp_vi_get_grid_sweeps")
        return k

    def values(self) -> np.ndarray:
        V = np.empty((self.B, self.S), self.np_dtype)
        _lib.check(self.L.mgdp_vi_get_values(self.h, _lib.ptr(V)), "mgdp_vi_get_values")
        return V

    def policy(self) -> np.ndarray:
        pi = np.empty((self.B, self.S), np.int8)
        _lib.check(self.L.mgdp_vi_get_policy(self.h, _lib.ptr(pi)), "mgdp_vi_get_policy")
        return pi

    # -- checkpoint / resume: Jacobi is memoryless given V_k
    def _ckpt_meta(self) -> dict:
        """What a checkpoint is only valid for: the grids (sha256 of the cells, None after
        load_device) and every parameter the Jacobi trajectory depends on."""
        d = self.desc
        return {"model": self.model, "dtype": self.dtype, "B": self.B, "W": self.W, "H": self.H,
                "gamma": float(d.gamma), "tol": float(d.tol), "slip_p": float(d.slip_p),
                "lava_mode": int(d.lava_mode), "death_cost": float(d.death_cost), "horizon": int(d.horizon),
                "cells_sha256": self._cells_digest}

    def checkpoint(self) -> dict:
        """The state of the last solve: {"V" (B, S), "pi" (B, S), "sweeps", "dv", "converged",
        "meta"}.  A solve stopped by max_sweeps before converging continues from it with resume()
        on a handle of the same grids and parameters whose max_sweeps is larger than the
        checkpoint's sweep count (so not on the capped handle itself), bit-identical to the
        uninterrupted solve."""
        return {"V": self.values(), "pi": self.policy(), "sweeps": int(self.sweeps), "dv": float(self.dv),
                "converged": bool(self.converged), "meta": self._ckpt_meta()}

    def resume(self, ckpt: dict, verify_cells: bool = True) -> int:
        """Continue from checkpoint() output (mgdp_vi_resume); returns the sweeps of the whole solve.
        Refused (ValueError): a converged checkpoint (final), V of another shape or dtype, a
        checkpoint of other grids or parameters (its "meta"), and with verify_cells a handle or
        checkpoint whose cells are unknown (loaded with load_device)."""
        V = _ckpt.resume_values(self._ckpt_meta(), ckpt, self.np_dtype, self.B, self.S, verify_cells)
        return self._call_result("mgdp_vi_resume", _lib.ptr(V), int(ckpt["sweeps"]), float(ckpt["dv"]))

    save_checkpoint = staticmethod(_ckpt.save_checkpoint)
    load_checkpoint = staticmethod(_ckpt.load_checkpoint)

    def dv_trace(self) -> np.ndarray:
        t = np.zeros(self.sweeps, np.float64)
        _lib.check(self.L.mgdp_vi_get_dv_trace(self.h, _lib.ptr(t), self.sweeps), "mgdp_vi_get_dv_trace")
        return t

    def result(self) -> VIResult:
        return VIResult(self.values(), self.policy(), self.sweeps, self.converged, self.dv, self.model,
                        self.W, self.H)

    def device_buffers(self) -> tuple[int, int]:
        """(V_ptr, pi_ptr): device pointers of the handle's V (B*S of its dtype) and pi (B*S int8) buffers
        (mgdp_vi_device_buffers), for zero-copy consumers such as MiniGridVecEnv.rollout_device.  The
        handle is synchronised first, so a resident lone-grid server's result is in HBM; the pointers
        stay valid until close() and are overwritten by the next solve / evaluate / improve."""
        self.synchronize()
        dV, dpi = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.L.mgdp_vi_device_buffers(self.h, ctypes.byref(dV), ctypes.byref(dpi)), "mgdp_vi_device_buffers")
        return int(dV.value or 0), int(dpi.value or 0)

    def synchronize(self):
        """Complete all work of the handle (a resident lone-grid server leaves, the stream drains)."""
        _lib.check(self.L.mgdp_vi_synchronize(self.h), "mgdp_vi_synchronize")

    def enable_timing(self, on: bool = True):
        _lib.check(self.L.mgdp_vi_enable_timing(self.h, int(on)), "mgdp_vi_enable_timing")

    def serve_clock(self) -> dict:
        """Shader clock of the persistent lone-grid servers that ran since enable_timing(): each
        launch's s_memtime cycles over its s_memrealtime lifetime (mgdp_vi_serve_clock)."""
        mhz, us, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        sus, ns = ctypes.c_double(), ctypes.c_int64()
        _lib.check(self.L.mgdp_vi_serve_clock(self.h, ctypes.byref(mhz), ctypes.byref(us), ctypes.byref(n),
                                              ctypes.byref(sus), ctypes.byref(ns)), "mgdp_vi_serve_clock")
        return {"sclk_mhz": mhz.value, "server_us": us.value, "launches": n.value, "gpu_solve_us": sus.value,
                "solves": ns.value}

    def _serve_path(self):
        path, counts = ctypes.c_int32(-1), (ctypes.c_int64 * 3)()
        _lib.check(self.L.mgdp_vi_serve_path(self.h, ctypes.byref(path), counts), "mgdp_vi_serve_path")
        return path.value, tuple(int(x) for x in counts)

    def serve_path(self) -> int:
        """The path the last served request took on the pair server (mgdp_vi_serve_path): 0 swept, 1 the
        depth form, 2 the depth form abandoned at a limit, then swept.  Asks a resident server to leave."""
        return self._serve_path()[0]

    def serve_path_counts(self) -> tuple[int, int, int]:
        """The handle's served requests by path (0, 1, 2), over the servers that have left; asks a resident
        server to leave, as serve_path() does."""
        return self._serve_path()[1]

    def kernel_time(self) -> tuple[float, int]:
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        _lib.check(self.L.mgdp_vi_kernel_time(self.h, ctypes.byref(ms), ctypes.byref(n)), "mgdp_vi_kernel_time")
        return ms.value, n.value

    @property
    def updates_per_sweep(self) -> int:
        return self.B * self.S * n_actions(self.model)


def policy_evaluation(grids, pi, **kwargs) -> VIResult:
    """V^pi of one policy per grid ((B, S) int8, see ValueIteration.evaluate) on one GPU; kwargs as
    ValueIteration (gamma, tol, slip_p, dtype, ...).  The result's pi is the evaluated policy."""
    vi = ValueIteration(grids, **kwargs)
    try:
        vi.evaluate_opts(pi)  # any handle: (H, B, S) accepted with a horizon
        return vi.result()
    finally:
        vi.close()


def policy_occupancy(grids, pi, start, n_steps: int | None = None, every_step: bool = False, **kwargs) -> OccupancyResult:
    """The forward pass of one policy per grid (ValueIteration.occupancy) on one GPU; kwargs as
    ValueIteration (gamma, slip_p, lava, death_cost, horizon, dtype, ...)."""
    vi = ValueIteration(grids, **kwargs)
    try:
        return vi.occupancy(pi, start, n_steps=n_steps, every_step=every_step)
    finally:
        vi.close()


def action_values(grids, pi=None, **kwargs) -> ActionValues:
    """Q*, or Q^pi of one policy per grid ((B, S) int8, see ValueIteration.evaluate), with the optimal-action
    sets, on one GPU; kwargs as ValueIteration (gamma, tol, slip_p, lava, dtype, ...)."""
    vi = ValueIteration(grids, **kwargs)
    try:
        if pi is None:
            vi.solve()
        else:
            vi.evaluate_opts(pi)
        Q, opt = vi.action_values(optimal=True)
        return ActionValues(Q, opt, vi.values(), vi.policy(), vi.sweeps, vi.model)
    finally:
        vi.close()


def policy_iteration(grids, pi0=None, max_iters: int = 1000, **kwargs) -> VIResult:
    """Policy iteration on one GPU (ValueIteration.policy_iteration); the result carries iters,
    eval_sweeps and changed, and its sweeps is the last evaluation's count."""
    vi = ValueIteration(grids, **kwargs)
    try:
        r = vi.policy_iteration_opts(pi0, max_iters=max_iters)
        out = vi.result()
        out.iters, out.eval_sweeps, out.changed = r["iters"], r["eval_sweeps"], r["changed"]
        return out
    finally:
        vi.close()


def value_iteration(grids, **kwargs) -> VIResult:
    """Solve value iteration for one grid or a batch (one global stopping rule) on one GPU."""
    vi = ValueIteration(grids, **kwargs)
    try:
        vi.solve()
        return vi.result()
    finally:
        vi.close()
