"""The two edges of a served solve around the pair loop: the pair loop's exit
reduction (one slot per wave, one 16-byte read, a wave of zeros skips its DPP chain) and the request's
way in, which every instantiation of vi_serve_kernel shares (the poller's word, plain requests, new cells
from host and device memory, a last solve, the idle limit).  Every case is a lone grid on the resident
server, against the CPU oracle bit for bit: sweeps, dV, V and pi.

A solve from V_0 = 0 of a deterministic grid sets a state n steps from the goal at sweep n, to gamma^(n-1),
and never changes it again: at any sweep every non-zero |dV| is the same number, so "the largest |dV| lies in
wave w" means that w is the only wave whose |dV| is not zero.  The corridor cases put that wave first,
in the middle and last; where it lies is asserted on the oracle's V_K and V_{K-1} alone, before any GPU
work."""
import functools
import time

import numpy as np
import pytest
import torch

import minigrid_dynamicprogramming_amd as mg
from oracle import oracle

pytestmark = pytest.mark.gpu

EMPTY, WALL, GOAL = 1, 2, 8
DTYPES = pytest.mark.parametrize("dtype", ["f32", "f64"])


def room(W, H, goals=(), walls=()):
    g = np.full((H, W), EMPTY, np.uint8)
    g[0, :] = g[-1, :] = WALL
    g[:, 0] = g[:, -1] = WALL
    for y, x in walls:
        g[y, x] = WALL
    for y, x in goals:
        g[y, x] = GOAL
    return g


def snake_path(W=16, H=16):
    """One corridor folded over the interior: odd rows in alternating directions, joined through the even rows."""
    path, right = [], True
    for y in range(1, H - 1, 2):
        xs = range(1, W - 1) if right else range(W - 2, 0, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H - 1:
            path.append((y + 1, W - 2 if right else 1))
        right = not right
    return path


def corridor(start, L):
    """16x16 of walls but for a goal at the fold's cell `start` and the L free cells after it.  A wave holds
    four rows: cells 0-29 of the fold lie in wave 0, 29-58 in wave 1, 59-88 in wave 2, 89-103 in wave 3."""
    g = np.full((16, 16), WALL, np.uint8)
    path = snake_path()
    for y, x in path[start + 1:start + L + 1]:
        g[y, x] = EMPTY
    g[path[start]] = GOAL
    return g


def empty16():
    enc, _ = mg.make("MiniGrid-Empty-16x16-v0").generate(seed=0)
    return np.ascontiguousarray(enc[:, :, 0].T)


def doorkey(env_id):
    enc, _ = mg.make(env_id).generate(seed=1)
    return np.ascontiguousarray(enc[:, :, 0].T).astype(np.uint8)


GRIDS = {
    "empty16": empty16,
    "8x8": lambda: room(8, 8, goals=[(6, 6)]),  # one wave
    "9x9": lambda: room(9, 9, goals=[(7, 7)]),  # two
    # 13x13, three: cells 127 | 128 are (9, 10) | (9, 11): a wall keeps that wave edge closed
    "13x13": lambda: room(13, 13, goals=[(11, 11)], walls=[(9, 11)]),
    "16x16": lambda: room(16, 16, goals=[(14, 14)]),  # four
    # rows 12..15 (the fourth wave) hold only walls: its |dV| is +0 at every stop
    "16x16_last_wave_walls": lambda: room(16, 16, goals=[(10, 13)], walls=[(y, x) for y in (12, 13, 14) for x in range(1, 15)]),
    # only rows 1..2 are open: one working wave on a four-wave workgroup
    "16x16_first_wave_only": lambda: room(16, 16, goals=[(2, 13)], walls=[(y, x) for y in range(3, 15) for x in range(1, 15)]),
    "other_goal": lambda: room(16, 16, goals=[(5, 9)]),
    # the largest |dV| of the stopping sweep in wave 0, in wave 1 (goal in wave 0) and in wave 3 (goal in wave 2)
    "corridor_w0": lambda: corridor(0, 30),
    "corridor_w1": lambda: corridor(27, 20),
    "corridor_w3": lambda: corridor(87, 16),
    "corridor_short": lambda: corridor(0, 3),  # wave 0 alone, at its fixed point after six sweeps
    # 20x12 without walls at the wave edges: serve_ew_ok fails, the pair server runs its fallback loop
    "20x12_open": lambda: room(20, 12, goals=[(10, 18)]),
    "doorkey8": lambda: doorkey("MiniGrid-DoorKey-8x8-v0"),
    "doorkey16": lambda: doorkey("MiniGrid-DoorKey-16x16-v0"),
}


@functools.lru_cache(maxsize=None)
def ref(key, dtype, gamma=0.99, tol=1e-6, max_sweeps=10000):
    """The oracle's solve, computed once per case, shared and left unchanged."""
    model = 1 if key.startswith("doorkey") else 0
    return oracle.value_iteration(model, GRIDS[key]()[None], gamma=gamma, tol=tol, max_sweeps=max_sweeps, dtype=dtype)


def wave_edge_open(g):
    """serve_ew_ok's rule for the grids of this file (walkable = EMPTY)."""
    flat = g.reshape(-1) == EMPTY
    return any(flat[c] and flat[c + 1] for c in range(63, flat.size - 1, 64))


def handle(g, dtype, monkeypatch, variant="serve_pair", env=(), **kw):
    monkeypatch.setenv("MGDP_PERSISTENT", "1")
    for name, value in env:
        monkeypatch.setenv(name, value)
    vi = mg.ValueIteration(g[None], dtype=dtype, **kw)
    assert vi.persistent and vi.variant == variant and "vi_serve_kernel" in vi.kernel_name
    return vi


def check_kdv(vi, o):
    assert vi.sweeps == o["sweeps"]
    assert vi.dv == o["dv"]


def check(vi, o):
    check_kdv(vi, o)
    np.testing.assert_array_equal(vi.values(), o["V"])  # reading V or pi stops the server
    np.testing.assert_array_equal(vi.policy(), o["pi"])


def waves_changing_at_stop(key, dtype, gamma, tol):
    """The waves whose cells hold the stopping sweep's largest |dV|, from the oracle's V_K and V_{K-1}."""
    o = ref(key, dtype, gamma=gamma, tol=tol)
    before = ref(key, dtype, gamma=gamma, tol=tol, max_sweeps=o["sweeps"] - 1)
    assert before["sweeps"] == o["sweeps"] - 1
    d = np.abs(o["V"].reshape(-1) - before["V"].reshape(-1))
    assert d.max() == o["dv"]
    return {int(s) // 4 // 64 for s in np.flatnonzero(d == d.max())}


@DTYPES
@pytest.mark.parametrize("name,block,env", [
    ("8x8", 64, (("MGDP_WAVE", "0"),)),  # the plan's one-wave loop switched off: the pair loop on one wave
    ("9x9", 128, ()), ("13x13", 192, ()), ("16x16", 256, ()), ("16x16_last_wave_walls", 256, ()),
    ("16x16_first_wave_only", 256, ()),
])
def test_one_to_four_waves_stop_at_a_fixed_point(name, block, env, dtype, monkeypatch):
    """The pair loop on 1, 2, 3 and 4 waves, and on four of which only some work: the slots of waves the
    workgroup does not have read as +0.  The stop is an exact fixed point (dV = 0.0: every wave stores +0
    without the DPP chain); two solves on one launch, the second on the slots the first left."""
    g, o = GRIDS[name](), ref(name, dtype)
    assert (g.size + 63) // 64 * 64 == block and not wave_edge_open(g)
    assert o["dv"] == 0.0 and o["sweeps"] > 6
    vi = handle(g, dtype, monkeypatch, env=env)
    try:
        vi.solve()
        check_kdv(vi, o)
        vi.solve()
        check(vi, o)
    finally:
        vi.close()


@DTYPES
@pytest.mark.parametrize("tol", [1e-2, 1e-3])
@pytest.mark.parametrize("name,wave", [("corridor_w0", 0), ("corridor_w1", 1), ("corridor_w3", 3)])
def test_largest_dv_in_each_wave_in_turn(name, wave, tol, dtype, monkeypatch):
    """gamma = 0.5 stops by tolerance on a sweep whose dV is 2^-(K-1), not zero (1e-2: K = 8, a pair's
    first sweep; 1e-3: K = 11, a second).  The one wave that still changes takes the DPP chain, the others
    the zero shortcut, in the same launch; the result comes out of that wave's slot."""
    g, o = GRIDS[name](), ref(name, dtype, gamma=0.5, tol=tol)
    assert not wave_edge_open(g)
    assert 0 < o["dv"] < tol and o["sweeps"] == (11 if tol == 1e-3 else 8)
    assert waves_changing_at_stop(name, dtype, 0.5, tol) == {wave}
    vi = handle(g, dtype, monkeypatch, gamma=0.5, tol=tol)
    try:
        vi.solve()
        check_kdv(vi, o)
        vi.solve()
        check(vi, o)
    finally:
        vi.close()


@DTYPES
@pytest.mark.parametrize("name", ["16x16_last_wave_walls", "empty16"])
def test_tolerance_stop_with_a_wave_of_zeros_beside_working_waves(name, dtype, monkeypatch):
    """gamma = 0.5 at 1e-3 on rooms: several waves change at the stop; on the first grid the last wave is all
    walls, so one launch takes both sides of the zero shortcut."""
    g, o = GRIDS[name](), ref(name, dtype, gamma=0.5, tol=1e-3)
    assert 0 < o["dv"] < 1e-3
    changing = waves_changing_at_stop(name, dtype, 0.5, 1e-3)
    assert len(changing) >= 2 and (name == "empty16" or 3 not in changing)
    vi = handle(g, dtype, monkeypatch, gamma=0.5, tol=1e-3)
    try:
        vi.solve()
        check_kdv(vi, o)
        vi.solve()
        check(vi, o)
    finally:
        vi.close()


@DTYPES
def test_no_stale_slot_after_a_grid_with_more_working_waves(dtype, monkeypatch):
    """One launch: a grid whose stop leaves a non-zero dV in wave 3's slot, then, loaded on the resident
    server, one that works in wave 0 only and stops with dV = 0.0, one that leaves its dV in wave 1's slot and
    a room whose first wave alone works.  Each dV is the grid's own."""
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "1000000")  # the server waits for the next request
    seq = ["corridor_w3", "corridor_short", "corridor_w1", "16x16_first_wave_only"]
    os_ = [ref(name, dtype, gamma=0.5, tol=1e-2) for name in seq]
    assert os_[0]["dv"] > 0 and os_[1]["dv"] == 0.0 and os_[2]["dv"] > 0 and os_[3]["dv"] > 0
    assert waves_changing_at_stop("16x16_first_wave_only", dtype, 0.5, 1e-2) == {0}
    vi = handle(GRIDS[seq[0]](), dtype, monkeypatch, gamma=0.5, tol=1e-2)
    try:
        for i, (name, o) in enumerate(zip(seq, os_)):
            if i:
                vi.load(GRIDS[name]()[None])
            vi.solve()
            check_kdv(vi, o)
            vi.solve()
            check_kdv(vi, o)
        clk = vi.serve_clock()  # stops the server
        assert clk["launches"] == 1 and clk["solves"] == 2 * len(seq)
        check(vi, os_[-1])
    finally:
        vi.close()


@DTYPES
def test_every_request_kind_on_one_launch(dtype, monkeypatch):
    """plain, plain, new cells from host memory, plain, new cells from a device pointer, plain, a last solve
    (the server leaves behind it), then a solve that has to relaunch.  K and dV after every request (reading
    V or pi would stop the server), V and pi where the server has left anyway."""
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "1000000")
    a, b, c = GRIDS["empty16"](), GRIDS["other_goal"](), GRIDS["16x16_last_wave_walls"]()
    oa, ob, oc = ref("empty16", dtype), ref("other_goal", dtype), ref("16x16_last_wave_walls", dtype)
    assert len({oa["sweeps"], ob["sweeps"], oc["sweeps"]}) == 3  # the grids tell themselves apart
    dev = torch.from_numpy(c).cuda()
    torch.cuda.synchronize()
    vi = handle(a, dtype, monkeypatch)
    try:
        vi.solve()
        check_kdv(vi, oa)
        vi.solve()
        check_kdv(vi, oa)
        vi.load(b[None])  # travels with the next request, from host memory
        vi.solve()
        check_kdv(vi, ob)
        vi.solve()
        check_kdv(vi, ob)
        vi.load_device(dev.data_ptr())  # ... from device memory
        vi.solve()
        check_kdv(vi, oc)
        vi.solve()
        check_kdv(vi, oc)
        vi.solve(last=True)
        check_kdv(vi, oc)
        vi.solve()  # relaunches
        check_kdv(vi, oc)
        clk = vi.serve_clock()
        assert clk["launches"] == 2 and clk["solves"] == 8
        check(vi, oc)
    finally:
        vi.close()


@DTYPES
def test_values_and_policy_behind_each_request_kind(dtype, monkeypatch):
    """The same kinds of request with V and pi read after each (the read stops the server, so each
    request here is also a launch's first)."""
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "1000000")
    a, b, c = GRIDS["empty16"](), GRIDS["other_goal"](), GRIDS["16x16_last_wave_walls"]()
    oa, ob, oc = ref("empty16", dtype), ref("other_goal", dtype), ref("16x16_last_wave_walls", dtype)
    dev = torch.from_numpy(c).cuda()
    torch.cuda.synchronize()
    vi = handle(a, dtype, monkeypatch)
    try:
        vi.solve()
        vi.solve()  # a plain request on a resident server
        check(vi, oa)
        vi.solve()
        vi.load(b[None])
        vi.solve()  # new cells from host memory on a resident server
        check(vi, ob)
        vi.solve()
        vi.load_device(dev.data_ptr())
        vi.solve()  # new cells from a device pointer on a resident server
        check(vi, oc)
        vi.solve()
        vi.solve(last=True)
        check(vi, oc)
    finally:
        vi.close()


@DTYPES
def test_idle_exit_and_relaunch(dtype, monkeypatch):
    """The default idle limit is 100 us: after a pause of milliseconds the poller alone has decided to leave
    and taken the other waves with it, and the next solve relaunches."""
    monkeypatch.delenv("MGDP_SERVE_IDLE_US", raising=False)
    o = ref("empty16", dtype)
    vi = handle(empty16(), dtype, monkeypatch)
    try:
        vi.solve()
        check_kdv(vi, o)
        time.sleep(0.005)
        vi.solve()
        check_kdv(vi, o)
        clk = vi.serve_clock()
        assert clk["launches"] == 2 and clk["solves"] == 2
        check(vi, o)
    finally:
        vi.close()


@DTYPES
@pytest.mark.parametrize("name,variant,env", [
    ("20x12_open", "serve_pair", ()),           # fails serve_ew_ok: the pair server's fallback loop
    ("8x8", "serve_wave", ()),                  # the one-wave served loop
    ("doorkey8", "serve_dk_half", ()),          # DoorKey, states over two threads
    ("doorkey16", "serve", (("MGDP_DK_HALF", "0"),)),  # DoorKey on the generic server
    ("16x16", "serve", (("MGDP_LONE_CPT", "2"),)),  # two cells per thread (Loop::xyd_x2: 128 threads, tests/test_vi_plan.py)
])
def test_other_served_loops_through_the_shared_entry(name, variant, env, dtype, monkeypatch):
    """Two plain solves on one launch on each of the other loops vi_serve_kernel is instantiated for."""
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "1000000")
    g, o = GRIDS[name](), ref(name, dtype)
    if name == "20x12_open":
        assert wave_edge_open(g)
    vi = handle(g, dtype, monkeypatch, variant=variant, env=env)
    try:
        vi.solve()
        check_kdv(vi, o)
        vi.solve()
        check_kdv(vi, o)
        clk = vi.serve_clock()
        assert clk["launches"] == 1 and clk["solves"] == 2
        check(vi, o)
    finally:
        vi.close()
