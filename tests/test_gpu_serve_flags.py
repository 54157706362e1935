"""The served pair loop's stop flags and tile layout (fused_serve_pair, csrc/vi_loops.h): each wave writes
the stop bits of a pair's two sweeps into one of two rotating flag slots, the next pair tests both, and a
cell's four planes lie side by side in the LDS tiles (one 16-byte access per cell for fp32, the cells
c + W and c - W read whole).  Every case is a lone grid of 65-256 cells on the resident server, against
the CPU oracle bit for bit: sweeps, dV, V and pi.

The loop is unrolled by six pairs (three register sets times two tiles) and a solve from V_0 = 0 makes
sweep 1 in registers, so the last sweep K >= 2 of a solve is made by the pair at loop position
((K - 2) // 2) % 6, as that pair's first sweep when K is even and as its second when K is odd (the pair
after it sees the flags and stops).  A family of corridors whose K
takes twelve or more consecutive values therefore meets every position with both kinds of stop; that
coverage is asserted on the oracle's K alone, before any GPU work."""
import functools

import numpy as np
import pytest

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


def empty16():
    enc, _ = mg.make("MiniGrid-Empty-16x16-v0").generate(seed=0)
    return np.ascontiguousarray(enc[:, :, 0].T)


def snake_path(W, H):
    """The cells of one corridor folded over the interior of a W x H grid, in walking order: odd rows
    left to right and right to left in turn, joined at alternating ends through the even rows."""
    path, right = [], True
    for y in range(1, H - 1, 2):
        xs = range(1, W - 1) if right else range(W - 2, 0, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H - 1:
            path.append((y + 1, W - 2 if right else 1))
        right = not right
    return path


def corridor(L, W=16, H=16):
    """Walls everywhere but the first L + 1 cells of the folded corridor: a goal, then L free cells."""
    g = np.full((H, W), WALL, np.uint8)
    path = snake_path(W, H)
    for y, x in path[1:L + 1]:
        g[y, x] = EMPTY
    g[path[0]] = GOAL
    return g


CORRIDORS = list(range(1, 31))  # the first two rows of the fold and the turn between them


@functools.lru_cache(maxsize=None)
def ref(key, dtype, gamma=0.99, tol=1e-6, max_sweeps=10000):
    """The oracle's solve, computed once per case, shared and left unchanged."""
    return oracle.value_iteration(0, GRIDS[key]()[None], gamma=gamma, tol=tol, max_sweeps=max_sweeps, dtype=dtype)


def wave_edge_open(g):
    """serve_ew_ok's rule for the grids of this file (walkable = EMPTY): some wave's last cell and the
    next wave's first are both walkable; then the server runs its fallback loop on the grid."""
    flat = g.reshape(-1) == EMPTY
    return any(flat[c] and flat[c + 1] for c in range(63, flat.size - 1, 64))


GRIDS = {f"corridor{L}": functools.partial(corridor, L) for L in CORRIDORS}
GRIDS.update({
    "empty16": empty16,
    "9x9": lambda: room(9, 9, goals=[(7, 7)]),
    # 13x13: cells 127 | 128 are (9, 10) | (9, 11): a wall keeps that wave edge closed
    "13x13": lambda: room(13, 13, goals=[(11, 11)], walls=[(9, 11)]),
    # rows 12..15 (the fourth wave) hold only walls
    "16x16_last_wave_walls": lambda: room(16, 16, goals=[(10, 13)], walls=[(y, x) for y in (12, 13, 14) for x in range(1, 15)]),
    # 20x12: 256 slots, pad 48, a plane stride of 352 elements (no multiple of 64); walls at the wave edges
    "20x12_closed": lambda: room(20, 12, goals=[(10, 18)], walls=[(3, 3), (6, 7), (9, 11)]),
    "20x12_open": lambda: room(20, 12, goals=[(10, 18)]),
    "goal_3_5": lambda: room(16, 16, goals=[(3, 5)]), "goal_4_9": lambda: room(16, 16, goals=[(4, 9)]),
    "goal_7_1": lambda: room(16, 16, goals=[(7, 1)]), "goal_8_14": lambda: room(16, 16, goals=[(8, 14)]),
    "goal_11_14": lambda: room(16, 16, goals=[(11, 14)]), "goal_12_1": lambda: room(16, 16, goals=[(12, 1)]),
})


def handle(g, dtype, monkeypatch, **kw):
    monkeypatch.setenv("MGDP_PERSISTENT", "1")
    vi = mg.ValueIteration(g[None], dtype=dtype, **kw)
    assert vi.persistent and vi.variant == "serve_pair"
    return vi


def check_kdv(vi, o):
    assert vi.sweeps == o["sweeps"]
    assert vi.dv == o["dv"]


def check(vi, o):
    check_kdv(vi, o)
    np.testing.assert_array_equal(vi.values(), o["V"])
    np.testing.assert_array_equal(vi.policy(), o["pi"])


def position(K):
    """(loop position of the pair that makes sweep K >= 2, 1 = as its first sweep / 2 = as its second)."""
    return ((K - 2) // 2) % 6, 2 if K % 2 else 1


def corridor_coverage(dtype):
    ks = sorted({ref(f"corridor{L}", dtype)["sweeps"] for L in CORRIDORS})
    run = best = 1
    for a, b in zip(ks, ks[1:]):
        run = run + 1 if b == a + 1 else 1
        best = max(best, run)
    return ks, best


@DTYPES
def test_corridors_meet_every_loop_position_and_both_stop_kinds(dtype, monkeypatch):
    """Corridors of 1..30 free cells in front of a goal, each solved twice on its own handle."""
    ks, longest = corridor_coverage(dtype)
    assert longest >= 12, ks
    assert {position(K) for K in ks if K >= 2} == {(p, s) for p in range(6) for s in (1, 2)}
    for L in CORRIDORS:
        g, o = corridor(L), ref(f"corridor{L}", dtype)
        assert 65 <= g.size <= 256 and not wave_edge_open(g)
        vi = handle(g, dtype, monkeypatch)
        try:
            vi.solve()
            check_kdv(vi, o)
            vi.solve()  # the slots and tiles as the first solve left them
            check(vi, o)
        finally:
            vi.close()


@DTYPES
@pytest.mark.parametrize("name", ["9x9", "empty16"])
def test_caps(name, dtype, monkeypatch):
    """max_sweeps 1..14: the cap ends the solve on every sweep of the first seven pairs."""
    g = GRIDS[name]()
    for cap in range(1, 15):
        o = ref(name, dtype, max_sweeps=cap)
        assert o["sweeps"] == cap and o["dv"] >= 1e-6
        vi = handle(g, dtype, monkeypatch, max_sweeps=cap)
        try:
            vi.solve()
            check_kdv(vi, o)
            vi.solve()
            check(vi, o)
        finally:
            vi.close()


@DTYPES
@pytest.mark.parametrize("name,block", [("9x9", 128), ("13x13", 192), ("16x16_last_wave_walls", 256)])
def test_fewer_than_four_working_waves(name, block, dtype, monkeypatch):
    """Two waves, three waves, and four of which the last holds only walls: the flag bytes of waves the
    workgroup does not have read as zero, and a wave of walls reports no change from the first sweep on."""
    g, o = GRIDS[name](), ref(name, dtype)
    assert (g.size + 63) // 64 * 64 == block and o["sweeps"] > 6 and not wave_edge_open(g)
    vi = handle(g, dtype, monkeypatch)
    try:
        vi.solve()
        check_kdv(vi, o)
        vi.solve()
        check(vi, o)
    finally:
        vi.close()


# neighbours differ in the parity of K and so in the stop kind, and in how many pairs they run
SEQUENCE = ["corridor20", "corridor11", "empty16", "corridor1", "corridor6", "corridor7", "corridor2"]  # K 25 14 29 4 9 10 5


@DTYPES
@pytest.mark.parametrize("n", [3, 5, 7])
def test_several_grids_on_one_launch(n, dtype, monkeypatch):
    """The first n grids of SEQUENCE on one launch of the server, each loaded by a new-cells request and
    solved twice: a request never sees the flag slots or the tiles of the one before it."""
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "1000000")  # the server waits for the next request
    seq = SEQUENCE[:n]
    os_ = [ref(name, dtype) for name in seq]
    for a, b in zip(os_, os_[1:]):
        assert a["sweeps"] % 2 != b["sweeps"] % 2
    vi = handle(GRIDS[seq[0]](), dtype, monkeypatch)
    try:
        for i, (name, o) in enumerate(zip(seq, os_)):
            if i:
                vi.load(GRIDS[name]()[None])
            vi.solve()
            check_kdv(vi, o)
            vi.solve()
            check_kdv(vi, o)
        clk = vi.serve_clock()  # stops the server
        assert clk["launches"] == 1 and clk["solves"] == 2 * n
        check(vi, os_[-1])
    finally:
        vi.close()


@DTYPES
@pytest.mark.parametrize("tol", [1e-3, 1e-2])
def test_stop_by_tolerance_while_values_move(tol, dtype, monkeypatch):
    """gamma = 0.5: sweep k's largest |dV| is 2^-(k-1), so the rule stops on a sweep whose dV is not zero
    (1e-3: K = 11, a pair's second sweep; 1e-2: K = 8, a first)."""
    o = ref("empty16", dtype, gamma=0.5, tol=tol)
    assert 0 < o["dv"] < tol and o["sweeps"] == (11 if tol == 1e-3 else 8)
    vi = handle(empty16(), dtype, monkeypatch, gamma=0.5, tol=tol)
    try:
        vi.solve()
        check_kdv(vi, o)
        vi.solve()
        check(vi, o)
    finally:
        vi.close()


@DTYPES
def test_stride_not_a_multiple_of_64_and_the_fallback(dtype, monkeypatch):
    """20x12 with walls at the wave edges runs the pair loop on tiles of 352 cells; without them
    serve_ew_ok fails and the same server falls back, then takes the pair loop up again."""
    closed, opened = GRIDS["20x12_closed"](), GRIDS["20x12_open"]()
    assert not wave_edge_open(closed) and wave_edge_open(opened)
    oc, oo = ref("20x12_closed", dtype), ref("20x12_open", dtype)
    vi = handle(closed, dtype, monkeypatch)
    try:
        for g, o in [(closed, oc), (opened, oo), (closed, oc)]:
            vi.load(g[None])
            vi.solve()
            check(vi, o)
            vi.solve()
            check(vi, o)
    finally:
        vi.close()


@DTYPES
@pytest.mark.parametrize("name", ["goal_3_5", "goal_4_9", "goal_7_1", "goal_8_14", "goal_11_14", "goal_12_1"])
def test_goal_next_to_a_wave_boundary(name, dtype, monkeypatch):
    """16x16: a wave holds four rows.  A goal in a wave's last row has its south neighbour in the next
    wave, one in a wave's first row its north neighbour in the wave above: those neighbours' values come
    from the 16-byte reads of the cells one row away."""
    g, o = GRIDS[name](), ref(name, dtype)
    assert not wave_edge_open(g)
    vi = handle(g, dtype, monkeypatch)
    try:
        vi.solve()
        check(vi, o)
    finally:
        vi.close()
