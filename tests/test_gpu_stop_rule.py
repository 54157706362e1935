"""The stopping rule at other discounts and tolerances, on every loop family.

At gamma = 0.99 and tol = 1e-6 a deterministic grid's largest |dV| is 0.99^(k-1) while its frontier
grows and exactly 0 afterwards, so it always stops at an exact fixed point, where V_K == V_{K-1}: a
`>` for the `>=` of a loop's `diff >= cf.tol`, or a stop taken one sweep late, would go unseen.  At
gamma = 0.5 the largest |dV| of sweep k is 2^-(k-1) exactly (both dtypes), so a tolerance picks the
stopping sweep, the solve ends with dV > 0 and V_K != V_{K-1}, and the host branches for "a batch
whose grids did not all end at fixed points" run without a cap.

Each case creates its handle under the knobs that select one family (plan_vi's precedence, the
table of tests/test_vi_plan.py), asserts vi.variant / kernel_name / persistent before solving, and
compares sweeps, dV, converged, V and pi with the oracle bit for bit; the property that makes the
parameters bite is asserted on the oracle's result first.
"""
import functools

import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from oracle import oracle
from oracle.numpy_vi import NumpyVI
from tests.golden_util import cells_from_enc, load
from tests.test_gpu_wave2 import random_grids

pytestmark = pytest.mark.gpu

KNOBS = ("MGDP_PERSISTENT", "MGDP_PAIR", "MGDP_QUAD", "MGDP_WAVE", "MGDP_CPT", "MGDP_LONE_CPT", "MGDP_PAIR2", "MGDP_WAVE2",
         "MGDP_WAVE2N", "MGDP_MIX", "MGDP_BAND", "MGDP_GK", "MGDP_BSERVE", "MGDP_SERVE_EW", "MGDP_SERVE_PAIR",
         "MGDP_SERVE_BAND", "MGDP_DK_1T", "MGDP_DK_HALF", "MGDP_DK_ROWS", "MGDP_SWEEP_PIPE", "MGDP_SWEEP_M",
         "MGDP_SWEEP_BLOCK", "MGDP_SWEEP_GRID", "MGDP_CHAIN", "MGDP_ORDER", "MGDP_LEARN_ORDER")
BOTH = ("f32", "f64")
B = 37  # batches: a multiple of nothing


# ---- grids ---------------------------------------------------------------------------------------
def snake(W, H):
    """One corridor folded over the whole interior (walls on every second interior row, the gap at
    alternating ends), the goal at its far end: the frontier grows for more sweeps than the ladders
    below need, on any shape."""
    g = np.full((H, W), 2, np.uint8)
    g[1:-1, 1:-1] = 1
    for i, y in enumerate(range(2, H - 1, 2)):
        g[y, 1:-1] = 2
        g[y, W - 2 if i % 2 == 0 else 1] = 1
    g[1, 1] = 8
    return g


def walled_goal(W, H):
    """A goal nobody can enter: walls on all four sides of it (K = 1, V = 0)."""
    g = np.full((H, W), 2, np.uint8)
    g[1:-1, 1:-1] = 1
    y, x = H // 2, W // 2
    g[y, x] = 8
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        if 0 < y + dy < H - 1 and 0 < x + dx < W - 1:
            g[y + dy, x + dx] = 2
    return g


def no_goal(W, H):
    g = np.full((H, W), 2, np.uint8)
    g[1:-1, 1:-1] = 1
    return g


@functools.lru_cache(maxsize=None)
def xyd_batch(W, H):
    """37 grids: random ones, the snake (the batch's longest frontier, so the ladder's K is the batch's
    K), a goal walled in and a grid with no goal (both stop at sweep 1 with V = 0)."""
    g = random_grids(B, W, H, seed=W * 31 + H, goals=1 + W % 3)
    g[5], g[11], g[23] = snake(W, H), walled_goal(W, H), no_goal(W, H)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def doorkey(size, n=None):
    g = np.stack([cells_from_enc(e) for e in load(f"grids_doorkey{size}.npz")["enc"]])[:n]
    g.setflags(write=False)
    return g


GRIDS = {
    "snake16": lambda: (0, snake(16, 16)[None]), "snake8": lambda: (0, snake(8, 8)[None]),
    "batch9x7": lambda: (0, xyd_batch(9, 7)), "batch16": lambda: (0, xyd_batch(16, 16)),
    "batch19": lambda: (0, xyd_batch(19, 19)),
    "dk16_lone": lambda: (1, doorkey(16, 1)), "dk16": lambda: (1, doorkey(16, B)), "dk8": lambda: (1, doorkey(8, B)),
}

# family -> (vi.variant, vi.kernel_name, vi.persistent, knobs, constructor arguments, grids, dtypes)
FUSED, SERVE = "vi_fused_kernel", "vi_serve_kernel"
FAMILIES = {
    # a lone XYD grid on the resident server
    "serve_pair": ("serve_pair", SERVE, True, "", {}, "snake16", BOTH),
    "serve_ew": ("serve_ew", SERVE, True, "MGDP_SERVE_PAIR=0", {}, "snake16", BOTH),
    "serve_band": ("serve_band", SERVE, True, "MGDP_SERVE_BAND=1", {}, "snake16", BOTH),
    "serve_wave_p1": ("serve_wave", SERVE, True, "", {}, "snake8", BOTH),
    "serve_wave_p4": ("serve_wave", SERVE, True, "MGDP_WAVE=8", {}, "snake16", BOTH),
    # ... launched
    "wave": ("wave", FUSED, False, "MGDP_PERSISTENT=0", {}, "snake8", BOTH),
    "xyd_soa_lone": ("xyd_soa", FUSED, False, "MGDP_PERSISTENT=0", {}, "snake16", BOTH),
    # batched XYD
    "wave2_p1": ("wave2", FUSED, False, "MGDP_BSERVE=0", {}, "batch9x7", BOTH),
    "wave2_p6": ("wave2", FUSED, False, "MGDP_BSERVE=0", {}, "batch19", BOTH),
    "wave2_served": ("wave2", FUSED, False, "", {}, "batch16", BOTH),  # the resident batch server
    "wave2n": ("wave2n", FUSED, False, "MGDP_WAVE2N=1", {}, "batch19", BOTH),
    "mix": ("mix", FUSED, False, "MGDP_MIX=1", {}, "batch16", ("f32",)),
    "band": ("band", FUSED, False, "MGDP_BAND=1", {}, "batch16", BOTH),
    "xyd_pair2": ("xyd_pair2", FUSED, False, "MGDP_WAVE2=0", {}, "batch16", BOTH),
    "xyd_x2": ("xyd_x2", FUSED, False, "MGDP_WAVE2=0 MGDP_PAIR2=0", {}, "batch16", BOTH),
    "xyd_x4": ("xyd_x4", FUSED, False, "MGDP_WAVE2=0 MGDP_CPT=4", {}, "batch16", BOTH),
    "xyd_soa_batch": ("xyd_soa", FUSED, False, "MGDP_WAVE2=0 MGDP_CPT=1", {}, "batch16", BOTH),
    "pair": ("pair", FUSED, False, "MGDP_PAIR=1", {}, "batch16", BOTH),
    "quad": ("quad", FUSED, False, "MGDP_QUAD=1", {}, "batch16", BOTH),
    # DoorKey
    "dk_half_lone": ("serve_dk_half", SERVE, True, "", {}, "dk16_lone", BOTH),
    "dk_half_batch": ("dk_half", FUSED, False, "", {}, "dk16", ("f64",)),
    "dk_rows": ("dk_rows", FUSED, False, "", {}, "dk16", ("f32",)),
    "dk_soa": ("dk_soa", FUSED, False, "", {}, "dk8", ("f32",)),
    "dk_1t": ("dk_1t", FUSED, False, "MGDP_DK_1T=1", {}, "dk16", ("f32",)),
    # both models: one thread per (state, action), and the per-sweep method's two kernels
    "sa_xyd_lone": ("sa", FUSED, False, "", {"mapping": "sa"}, "snake16", BOTH),
    "sa_xyd_batch": ("sa", FUSED, False, "", {"mapping": "sa"}, "batch16", BOTH),
    "sa_dk": ("sa", FUSED, False, "", {"mapping": "sa"}, "dk8", BOTH),
    "sweep_xyd": ("sweep", "vi_sweep_kernel", False, "MGDP_SWEEP_PIPE=0", {"method": "sweep"}, "batch16", BOTH),
    "sweep_pipe_xyd": ("sweep_pipe", "vi_sweep_pipe_kernel", False, "", {"method": "sweep"}, "batch16", BOTH),
    "sweep_dk": ("sweep", "vi_sweep_kernel", False, "", {"method": "sweep"}, "dk8", BOTH),
    "sweep_pipe_dk": ("sweep_pipe", "vi_sweep_pipe_kernel", False, "MGDP_SWEEP_PIPE=2", {"method": "sweep"}, "dk8", BOTH),
}
LONE = [f for f, r in FAMILIES.items() if r[5] in ("snake16", "snake8", "dk16_lone")]
BATCHED = [f for f in FAMILIES if f not in LONE]
XYD_BATCHED = [f for f in BATCHED if FAMILIES[f][5].startswith("batch")]


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def grids_of(family):
    return GRIDS[FAMILIES[family][5]]()


@functools.lru_cache(maxsize=None)
def ref(gkey, dtype, gamma, tol, max_sweeps=10000):
    """The oracle's solve: computed once per (grids, dtype, gamma, tol), shared and left unchanged."""
    model, cells = GRIDS[gkey]()
    return oracle.value_iteration(model, cells, gamma=gamma, tol=tol, max_sweeps=max_sweeps, dtype=dtype, fixed_point=True)


def handle(family, dtype, monkeypatch, cells=None, **kw):
    variant, kernel, persistent, knobs, ctor, _g, _d = FAMILIES[family]
    for kv in knobs.split():
        monkeypatch.setenv(*kv.split("="))
    model, own = grids_of(family)
    vi = mg.ValueIteration(own if cells is None else cells, model=("xyd", "doorkey")[model], dtype=dtype, **ctor, **kw)
    try:
        assert (vi.variant, vi.kernel_name, vi.persistent) == (variant, kernel, persistent)
    except BaseException:
        vi.close()
        raise
    return vi


def check(vi, o, tol, grid_sweeps):
    assert vi.sweeps == o["sweeps"]
    assert vi.dv == o["dv"]
    assert vi.converged == (o["dv"] < tol)
    np.testing.assert_array_equal(vi.values(), o["V"])
    np.testing.assert_array_equal(vi.policy(), o["pi"])
    if grid_sweeps:
        np.testing.assert_array_equal(vi.grid_sweeps(), o["grid_sweeps"])


def solve_and_check(family, dtype, monkeypatch, gamma, tol, o, solves=1):
    vi = handle(family, dtype, monkeypatch, gamma=gamma, tol=tol)
    try:
        for _ in range(solves):
            vi.solve()
        if family == "wave2_served":
            assert vi.serve_clock()["solves"] >= 1  # the batch server answered (this stops it)
        # a fused handle reports each grid's own sweeps; the sweep method reports K for every grid
        check(vi, o, tol, grid_sweeps=FAMILIES[family][4].get("method") != "sweep")
    finally:
        vi.close()


def solves_of(family):
    return 3 if family == "wave2_served" else 1


# ---- the ladder: gamma 0.5, tol = 1.5 * 2^-j -> K = j + 1 with dV = 2^-j > 0 ------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_ladder_of_tolerances(family, monkeypatch):
    """Every stopping sweep from 2 to 13 (both parities of the LDS ping-pong) on the lone families,
    sweeps 2, 3, 9 and 10 on the batched ones; the tolerances are exact in fp32."""
    gkey = FAMILIES[family][5]
    for dtype in FAMILIES[family][6]:
        for j in (range(1, 13) if family in LONE else (1, 2, 8, 9)):
            tol = 1.5 * 2.0 ** -j
            o = ref(gkey, dtype, 0.5, tol)
            assert o["sweeps"] == j + 1 and o["dv"] == 2.0 ** -j and 0 < o["dv"] < tol
            solve_and_check(family, dtype, monkeypatch, 0.5, tol, o, solves_of(family))


# ---- dV == tol does not stop; tol rounds up to the value type -------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_equality_and_tolerance_round_up(family, monkeypatch):
    """tol = 2^-j: the sweep with dV == tol goes on (K = j + 2).  tol = the next double above 2^-j:
    K = j + 1; as a float that tolerance rounds DOWN to 2^-j, which make_coef's nextafter undoes."""
    gkey = FAMILIES[family][5]
    for dtype in FAMILIES[family][6]:
        for j in (9, 10):
            tol = 2.0 ** -j
            o = ref(gkey, dtype, 0.5, tol)
            assert o["sweeps"] == j + 2 and o["dv"] == 2.0 ** -(j + 1)
            solve_and_check(family, dtype, monkeypatch, 0.5, tol, o, solves_of(family))
            up = float(np.nextafter(tol, 1.0))
            assert up > tol and float(np.float32(up)) == tol
            o = ref(gkey, dtype, 0.5, up)
            assert o["sweeps"] == j + 1 and o["dv"] == tol
            solve_and_check(family, dtype, monkeypatch, 0.5, up, o, solves_of(family))


@pytest.mark.parametrize("family", ["wave", "xyd_soa_lone", "sa_xyd_lone"])
def test_lone_launch_stops_where_the_rule_stops(family, monkeypatch):
    """The host repeats the rule on the launch's result (`while (!(dv < tol)) sweep`), so a kernel
    that stopped one sweep early at dV == tol (`>` for `>=`) would still give the right answer, one
    launch later.  A lone grid's own rule IS the global rule, so its launch must be the whole solve:
    one timed launch per solve."""
    for dtype in BOTH:
        for j in (9, 10):
            tol = 2.0 ** -j
            o = ref(FAMILIES[family][5], dtype, 0.5, tol)
            assert o["sweeps"] == j + 2 and o["dv"] == 2.0 ** -(j + 1)
            vi = handle(family, dtype, monkeypatch, gamma=0.5, tol=tol)
            try:
                vi.enable_timing(True)
                for _ in range(2):
                    vi.solve()
                assert vi.kernel_time()[1] == 2
                check(vi, o, tol, grid_sweeps=True)
            finally:
                vi.close()


# ---- the ends of the range ------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_ends_of_the_range(family, monkeypatch):
    gkey = FAMILIES[family][5]
    for dtype in FAMILIES[family][6]:
        o = ref(gkey, dtype, 0.0, 1e-6)  # gamma 0: only the step into the goal is worth anything
        assert o["sweeps"] == 2 and o["dv"] == 0.0 and set(np.unique(o["V"])) == {0.0, 1.0}
        solve_and_check(family, dtype, monkeypatch, 0.0, 1e-6, o, solves_of(family))
        o = ref(gkey, dtype, 0.999, 1e-6)
        assert o["dv"] == 0.0 and o["sweeps"] > 13
        solve_and_check(family, dtype, monkeypatch, 0.999, 1e-6, o, solves_of(family))
        o = ref(gkey, dtype, 0.99, 2.0)  # the first sweep's dV = 1 is already below tol
        assert o["sweeps"] == 1 and o["dv"] == 1.0
        solve_and_check(family, dtype, monkeypatch, 0.99, 2.0, o, solves_of(family))
        o = ref(gkey, dtype, 0.99, 1.0)  # ... and equal to it: one more sweep
        assert o["sweeps"] == 2 and o["dv"] == float(np.dtype(o["V"].dtype).type(0.99))
        solve_and_check(family, dtype, monkeypatch, 0.99, 1.0, o, solves_of(family))


# ---- batches mixing fixed-point and tolerance-stopped grids ---------------------------------------
def own_stops(model, cells, dtype, gamma, tol):
    own = [oracle.value_iteration(model, c, gamma=gamma, tol=tol, dtype=dtype) for c in cells]
    return np.array([o["sweeps"] for o in own]), np.array([o["dv"] for o in own])


@pytest.mark.parametrize("family", XYD_BATCHED)
def test_batch_of_fixed_point_and_tolerance_stops(family, monkeypatch):
    """Plain random grids at gamma 0.5 and a tolerance near the middle of their own fixed-point sweeps
    (9x7: tol 1e-3, K = 11; 16x16: 1.5 * 2^-28, K = 29; 19x19: 1.5 * 2^-38, K = 39): some grids end at
    exact fixed points (dV = 0) before K, the others by the tolerance (dV = 2^-(K-1)), so the launch's
    own rule leaves the batch at several sweeps and the host takes it to K."""
    _v, _k, _p, _kn, _c, gkey, dtypes = FAMILIES[family]
    W, H, tol, K = {"batch9x7": (9, 7, 1e-3, 11), "batch16": (16, 16, 1.5 * 2.0 ** -28, 29),
                    "batch19": (19, 19, 1.5 * 2.0 ** -38, 39)}[gkey]
    cells = random_grids(B, W, H, seed=W * 31 + H)
    for dtype in dtypes:
        k_own, dv_own = own_stops(0, cells, dtype, 0.5, tol)
        assert (dv_own > 0).sum() >= 5 and (dv_own == 0).sum() >= 5 and len(set(k_own.tolist())) >= 5
        o = oracle.value_iteration(0, cells, gamma=0.5, tol=tol, dtype=dtype, fixed_point=True)
        assert o["sweeps"] == K and o["dv"] == 2.0 ** -(K - 1)
        vi = handle(family, dtype, monkeypatch, cells=cells, gamma=0.5, tol=tol)
        try:
            for _ in range(solves_of(family)):
                vi.solve()
            check(vi, o, tol, grid_sweeps=FAMILIES[family][4].get("method") != "sweep")
        finally:
            vi.close()


@pytest.mark.parametrize("family", [f for f in BATCHED if FAMILIES[f][5] in ("dk8", "dk16")])
def test_doorkey_batch_of_fixed_point_and_tolerance_stops(family, monkeypatch):
    _v, _k, _p, _kn, _c, gkey, dtypes = FAMILIES[family]
    size, gamma, tol, K = {"dk8": (8, 0.7, 1e-3, 21), "dk16": (16, 0.5, 1.5 * 2.0 ** -9, 10)}[gkey]
    cells = doorkey(size)  # all 64 grids of the fixture
    for dtype in dtypes:
        k_own, dv_own = own_stops(1, cells, dtype, gamma, tol)
        if size == 8:
            assert (dv_own > 0).sum() >= 5 and (dv_own == 0).sum() >= 5
        else:
            assert (dv_own > 0).all() and (k_own == K).all()
        o = oracle.value_iteration(1, cells, gamma=gamma, tol=tol, dtype=dtype, fixed_point=True)
        assert o["sweeps"] == K and 0 < o["dv"] < tol
        vi = handle(family, dtype, monkeypatch, cells=cells, gamma=gamma, tol=tol)
        try:
            vi.solve()
            check(vi, o, tol, grid_sweeps=FAMILIES[family][4].get("method") != "sweep")
        finally:
            vi.close()


# ---- fp32 subnormals ------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [f for f in XYD_BATCHED if FAMILIES[f][5] != "batch9x7"])
def test_fp32_subnormal_values(family, monkeypatch):
    """gamma 0.05: V = 0.05^d drops below FLT_MIN from d = 30 on (no 9x7 grid is that deep); the
    oracle keeps subnormals, so the device must not flush them (a mismatch is a build-flag finding,
    not a tolerance)."""
    gkey = FAMILIES[family][5]
    o = ref(gkey, "f32", 0.05, 1e-44)
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((o["V"] > 0) & (o["V"] < tiny)).sum() >= 100
    solve_and_check(family, "f32", monkeypatch, 0.05, 1e-44, o, solves_of(family))


# ---- degenerate grids -----------------------------------------------------------------------------
def tiny3x4():
    g = np.full((4, 3), 2, np.uint8)  # W = 3, H = 4: one floor cell above the goal
    g[1, 1], g[2, 1] = 1, 8
    return g


def tiny3x3():
    g = np.full((3, 3), 2, np.uint8)
    g[1, 1] = 8
    return g


DEGENERATE = {
    "walled_goal": (lambda: walled_goal(9, 9), 1), "no_goal": (lambda: no_goal(9, 9), 1),
    "3x3": (tiny3x3, 1), "3x4": (tiny3x4, 4),
    "corridor_3x40": (lambda: snake(3, 40), None), "corridor_40x3": (lambda: snake(40, 3), None),
}
# (knobs, constructor arguments, vi.variant of a grid of <= 64 cells, of a larger one): the default plan,
# the launched kernels, SA and the sweep method, for a lone grid and for a batch
DEGENERATE_PLANS = {
    True: [("", {}, "serve_wave", "serve_pair"), ("MGDP_PERSISTENT=0", {}, "wave", "xyd_soa"),
           ("", {"mapping": "sa"}, "sa", "sa"), ("", {"method": "sweep"}, "sweep_pipe", "sweep_pipe")],
    False: [("", {}, "wave2", "wave2"), ("MGDP_WAVE2=0", {}, "xyd_pair2", "xyd_pair2"),
            ("MGDP_WAVE2=0 MGDP_CPT=1", {}, "xyd_soa", "xyd_soa"), ("", {"mapping": "sa"}, "sa", "sa"),
            ("", {"method": "sweep"}, "sweep_pipe", "sweep_pipe")],
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_grids_alone_and_in_a_batch(name, monkeypatch):
    make, K = DEGENERATE[name]
    g = make()
    H, W = g.shape
    batch = np.full((B, H, W), 2, np.uint8)
    if min(W, H) > 4:
        batch[:] = random_grids(B, W, H, seed=3)
    elif max(W, H) > 4:  # corridors: the goal at different depths (random cells would only add walls)
        for i in range(B):
            batch[i] = np.where(g == 8, 1, g)
            batch[i][(1 + i % (H - 2), 1) if W == 3 else (1, 1 + i % (W - 2))] = 8
    else:
        batch[:] = g
    batch[7] = g
    for gamma, tol in ((0.99, 1e-6), (0.5, 1e-3)):
        for cells in (g[None], batch):
            for dtype in BOTH:
                o = oracle.value_iteration(0, cells, gamma=gamma, tol=tol, dtype=dtype)
                own = oracle.value_iteration(0, g, gamma=gamma, tol=tol, dtype=dtype)
                if K is not None:
                    assert own["sweeps"] == K and (K > 1 or not own["V"].any())
                else:
                    assert own["sweeps"] >= 11  # the corridor's frontier outlasts the tolerance
                for knobs, ctor, small, large in DEGENERATE_PLANS[len(cells) == 1]:
                    for name_ in KNOBS:
                        monkeypatch.delenv(name_, raising=False)
                    for kv in knobs.split():
                        monkeypatch.setenv(*kv.split("="))
                    vi = mg.ValueIteration(cells, model="xyd", dtype=dtype, gamma=gamma, tol=tol, **ctor)
                    try:
                        assert vi.variant == (small if W * H <= 64 else large)
                        vi.solve()
                        check(vi, o, tol, grid_sweeps=False)
                    finally:
                        vi.close()


@pytest.mark.parametrize("family", [f for f in LONE if FAMILIES[f][5].startswith("snake")])
def test_lone_families_on_grids_with_nothing_to_find(family, monkeypatch):
    """A goal walled in, and no goal: the first sweep's dV is 0, so K = 1 and V = 0 (the batched
    families hold both grids in every batch above)."""
    W = H = 16 if FAMILIES[family][5] == "snake16" else 8
    for g in (walled_goal(W, H), no_goal(W, H)):
        for dtype in BOTH:
            for gamma, tol in ((0.99, 1e-6), (0.5, 1e-3)):
                o = oracle.value_iteration(0, g, gamma=gamma, tol=tol, dtype=dtype, fixed_point=True)
                assert o["sweeps"] == 1 and o["dv"] == 0.0 and not o["V"].any()
                vi = handle(family, dtype, monkeypatch, cells=g[None], gamma=gamma, tol=tol)
                try:
                    vi.solve()
                    check(vi, o, tol, grid_sweeps=True)
                finally:
                    vi.close()


# ---- the second reference -------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["serve_pair", "wave2_p6"])
def test_numpy_restatement_agrees(family, monkeypatch):
    """oracle/numpy_vi.py, the independent statement of the loop, on one lone and one batched case."""
    model, cells = grids_of(family)
    for dtype in BOTH:
        tol = 1.5 * 2.0 ** -9
        o = ref(FAMILIES[family][5], dtype, 0.5, tol)
        n = NumpyVI(model, cells, gamma=0.5, tol=tol, dtype=dtype).solve()
        assert n["sweeps"] == o["sweeps"] == 10 and n["dv"] == o["dv"]
        np.testing.assert_array_equal(n["V"], o["V"])
        np.testing.assert_array_equal(n["pi"], o["pi"])
        vi = handle(family, dtype, monkeypatch, gamma=0.5, tol=tol)
        try:
            vi.solve()
            check(vi, n, tol, grid_sweeps=False)
        finally:
            vi.close()
