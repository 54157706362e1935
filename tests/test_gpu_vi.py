"""GPU value iteration (csrc/vi.hip through the C ABI) vs the CPU oracle and the reference fixtures.

Bit-exact: sweeps, pi and V (same dtype, same operation order, no FMA contraction on either side).
Against the reference-derived golden V*/pi* (numpy fp64 Jacobi over transition tables extracted
from reference step()): identical sweeps and pi, V within 1e-12 (fp64) / 1e-6 (fp32).
"""
import numpy as np
import pytest

import minigrid_dynamicprogramming_amd as mg
from oracle import oracle
from tests.golden_util import cells_from_enc, load, table_names

pytestmark = pytest.mark.gpu

VARIANTS = [(m, p) for m in ("fused", "sweep") for p in ("cell", "sa")]


def gpu_vi(cells, model, dtype="f64", method="fused", mapping="cell", slip=None, **kw):
    return mg.value_iteration(cells, model=model, dtype=dtype, method=method, mapping=mapping,
                              slip_p=slip, **kw)


@pytest.mark.parametrize("method,mapping", VARIANTS)
@pytest.mark.parametrize("name", table_names())
def test_golden_tables_fp64(name, method, mapping):
    t = load(f"table_{name}.npz")
    model = "xyd" if int(t["model"]) == 0 else "doorkey"
    cells = cells_from_enc(t["enc"])
    r = gpu_vi(cells, model, "f64", method, mapping)
    assert r.sweeps == int(t["sweeps"]) and r.converged
    np.testing.assert_array_equal(r.pi[0], t["pi"])
    np.testing.assert_allclose(r.V[0], t["V"], rtol=0, atol=1e-12)
    o = oracle.value_iteration(int(t["model"]), cells, dtype="f64")
    np.testing.assert_array_equal(r.V[0], o["V"][0])  # bit-exact vs the oracle
    if model == "xyd":
        rs = gpu_vi(cells, model, "f64", method, mapping, slip=0.9)
        assert rs.sweeps == int(t["sweeps_slip"])
        np.testing.assert_array_equal(rs.pi[0], t["pi_slip"])
        np.testing.assert_allclose(rs.V[0], t["V_slip"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("method,mapping", VARIANTS)
@pytest.mark.parametrize("slip", [None, 0.9])
@pytest.mark.parametrize("name", ["empty16_s0", "fourrooms_s1", "lava11n5_s0", "doorkey16_s0", "doorkey8_s2"])
def test_fp32_bit_exact_vs_oracle(name, slip, method, mapping):
    t = load(f"table_{name}.npz")
    model_id = int(t["model"])
    if slip is not None and model_id == 1:
        pytest.skip("slip is defined for the XYD model")
    cells = cells_from_enc(t["enc"])
    r = gpu_vi(cells, "xyd" if model_id == 0 else "doorkey", "f32", method, mapping, slip=slip)
    o = oracle.value_iteration(model_id, cells, slip_p=slip, dtype="f32")
    assert r.sweeps == o["sweeps"]
    np.testing.assert_array_equal(r.pi, o["pi"])
    np.testing.assert_array_equal(r.V, o["V"])
    ref_V = t["V"] if slip is None else t["V_slip"]
    np.testing.assert_allclose(r.V[0], ref_V, rtol=0, atol=1e-6)  # north-star tolerance on V


@pytest.mark.parametrize("method,mapping", VARIANTS)
@pytest.mark.parametrize("env", ["fourrooms", "lava11n5", "doorkey16", "doorkey8"])
def test_batched_global_rule_vs_oracle(env, method, mapping):
    g = load(f"grids_{env}.npz")
    cells = np.stack([cells_from_enc(e) for e in g["enc"]])
    model = "doorkey" if env.startswith("doorkey") else "xyd"
    for dtype in ("f32", "f64"):
        r = gpu_vi(cells, model, dtype, method, mapping)
        o = oracle.value_iteration(0 if model == "xyd" else 1, cells, dtype=dtype)
        assert r.sweeps == o["sweeps"]
        np.testing.assert_array_equal(r.pi, o["pi"])
        np.testing.assert_array_equal(r.V, o["V"])


def test_slip_batched_fp32_vs_oracle():
    g = load("grids_lava11n5.npz")
    cells = np.stack([cells_from_enc(e) for e in g["enc"]])
    for method in ("fused", "sweep"):
        r = gpu_vi(cells, "xyd", "f32", method, "cell", slip=0.9)
        o = oracle.value_iteration(0, cells, slip_p=0.9, dtype="f32")
        assert r.sweeps == o["sweeps"]
        np.testing.assert_array_equal(r.V, o["V"])
        np.testing.assert_array_equal(r.pi, o["pi"])


def test_max_sweeps_cap_and_not_converged():
    t = load("table_empty16_s0.npz")
    cells = cells_from_enc(t["enc"])
    for method in ("fused", "sweep"):
        r = gpu_vi(cells, "xyd", "f64", method, max_sweeps=10)
        o = oracle.value_iteration(0, cells, max_sweeps=10)
        assert r.sweeps == 10 and not r.converged
        np.testing.assert_array_equal(r.V, o["V"])
        np.testing.assert_array_equal(r.pi, o["pi"])


def test_repeated_solves_identical():
    t = load("table_fourrooms_s0.npz")
    vi = mg.ValueIteration(cells_from_enc(t["enc"]), dtype="f32")
    vi.solve()
    V0 = vi.values()
    for _ in range(3):
        vi.solve()
        np.testing.assert_array_equal(vi.values(), V0)
    vi.close()


def test_known_answer_empty16_single_env():
    env = mg.make("MiniGrid-Empty-16x16-v0")
    env.generate(seed=0)
    r = mg.value_iteration(env.grid.cells()[None], dtype="f64")
    assert r.sweeps == 29
    assert r.value(0, 1, 1, 0) == pytest.approx(0.99 ** 26, abs=1e-15)


def test_full_size_replicas_property():
    # Empty-16x16 x 65536 replicas; every replica equals the single-env solution
    env = mg.make("MiniGrid-Empty-16x16-v0")
    env.generate(seed=0)
    one = env.grid.cells()
    cells = np.broadcast_to(one, (65536,) + one.shape).copy()
    single = mg.value_iteration(one[None], dtype="f32")
    for method in ("fused", "sweep"):
        vi = mg.ValueIteration(cells, dtype="f32", method=method)
        assert vi.solve() == 29
        V = vi.values()
        assert (V == single.V[0]).all()
        vi.close()


def test_invalid_grids_raise():
    bad = np.full((1, 5, 5), 2, np.uint8)
    bad[0, 2, 2] = 6  # ball: outside the XYD model
    with pytest.raises(ValueError):
        mg.value_iteration(bad, model="xyd")
    open_border = np.full((1, 5, 5), 2, np.uint8)
    open_border[0, 0, 2] = 1
    with pytest.raises(ValueError):
        mg.value_iteration(open_border, model="xyd")


@pytest.mark.parametrize("pair,quad,cpt", [("0", "0", "1"), ("0", "0", "2"), ("0", "0", "4"), ("1", "0", "1"), ("0", "1", "1")])
@pytest.mark.parametrize("slip", [None, 0.9])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fused_xyd_variants_bit_exact(pair, quad, cpt, slip, dtype, monkeypatch):
    """Every fused XYD loop -- one thread per cell, two cells per thread on batches (MGDP_CPT=2),
    the two-sweep step (3 LDS buffers), four threads per cell with DPP quad exchange -- agrees with
    the oracle bit for bit (batches of 7 and 64 grids with different own stopping sweeps also run
    the advance-to-K loop)."""
    monkeypatch.setenv("MGDP_PAIR", pair)
    monkeypatch.setenv("MGDP_QUAD", quad)
    monkeypatch.setenv("MGDP_CPT", cpt)
    for env in ("fourrooms", "lava11n5"):
        g = load(f"grids_{env}.npz")
        cells = np.stack([cells_from_enc(e) for e in g["enc"]])
        for sub in (cells[:1], cells[:7], cells):
            r = gpu_vi(sub, "xyd", dtype, "fused", "cell", slip=slip)
            o = oracle.value_iteration(0, sub, slip_p=slip, dtype=dtype)
            assert r.sweeps == o["sweeps"]
            np.testing.assert_array_equal(r.V, o["V"])
            np.testing.assert_array_equal(r.pi, o["pi"])
    t = load("table_empty16_s0.npz")
    for ms in (1, 2, 9, 10, 11):  # odd/even caps end on a one-sweep step
        r = gpu_vi(cells_from_enc(t["enc"]), "xyd", dtype, "fused", "cell", slip=slip, max_sweeps=ms)
        o = oracle.value_iteration(0, cells_from_enc(t["enc"]), slip_p=slip, dtype=dtype, max_sweeps=ms)
        assert r.sweeps == o["sweeps"] == ms
        np.testing.assert_array_equal(r.V, o["V"])
        np.testing.assert_array_equal(r.pi, o["pi"])


def _solve_one(cells, dtype="f32", **kw):
    vi = mg.ValueIteration(cells, dtype=dtype, **kw)
    vi.solve()
    out = (vi.sweeps, vi.values(), vi.policy())
    vi.close()
    return out


@pytest.mark.parametrize("pollers", ["1", "4"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_persistent_server_matches_launches(dtype, pollers, monkeypatch):
    """A lone grid is solved by the resident vi_serve_kernel (one or four waves polling the
    request word, MGDP_SERVE_POLLERS); it agrees bit for bit with one fused launch per solve
    (MGDP_PERSISTENT=0) and with the oracle."""
    monkeypatch.setenv("MGDP_SERVE_POLLERS", pollers)
    for name in ("empty16_s0", "fourrooms_s1", "lava11n5_s0", "doorkey8_s2", "doorkey16_s0"):
        t = load(f"table_{name}.npz")
        cells = cells_from_enc(t["enc"])[None]
        monkeypatch.setenv("MGDP_PERSISTENT", "1")
        k1, V1, p1 = _solve_one(cells, dtype)
        monkeypatch.setenv("MGDP_PERSISTENT", "0")
        k0, V0, p0 = _solve_one(cells, dtype)
        o = oracle.value_iteration(int(t["model"]), cells, dtype=dtype)
        assert k1 == k0 == o["sweeps"]
        np.testing.assert_array_equal(V1, V0)
        np.testing.assert_array_equal(p1, p0)
        np.testing.assert_array_equal(V1, o["V"])
        np.testing.assert_array_equal(p1, o["pi"])


def test_persistent_server_requests_and_handoffs(monkeypatch):
    """Back-to-back requests, new grids loaded between requests, result reads between requests, the
    multi-device protocol pieces after a served solve, and a server that idled out (relaunched by
    the host when the next request finds the stream empty)."""
    import time

    monkeypatch.setenv("MGDP_PERSISTENT", "1")
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "500")
    g = load("grids_fourrooms.npz")
    cells = [cells_from_enc(e)[None] for e in g["enc"][:6]]
    want = [oracle.value_iteration(0, c, dtype="f32") for c in cells]
    vi = mg.ValueIteration(cells[0], dtype="f32")
    for rep in range(3):
        for i, c in enumerate(cells):
            vi.load(c)
            assert vi.solve() == want[i]["sweeps"]
            assert vi.solve() == want[i]["sweeps"]  # back to back on the same grid
            if (i + rep) % 2 == 0:
                np.testing.assert_array_equal(vi.values(), want[i]["V"])
                np.testing.assert_array_equal(vi.policy(), want[i]["pi"])
            if i == 2:
                time.sleep(0.02)  # the server leaves after 0.5 ms idle
    # protocol pieces after a served solve (one device: the local rule is the global rule)
    vi.load(cells[1])
    vi.reset()
    k = vi.run_local()
    assert k == want[1]["sweeps"]
    assert vi.run_to(k) < vi.tol
    vi.finish(k, 0.0)
    np.testing.assert_array_equal(vi.values(), want[1]["V"])
    # timing: one resident launch serves every timed request
    vi.enable_timing(True)
    for _ in range(10):
        vi.solve()
    ms, n = vi.kernel_time()
    assert 1 <= n <= 3 and ms > 0  # one launch unless a scheduling hiccup outlasted the 0.5 ms idle limit
    vi.close()


def test_synchronize_ends_the_server_and_results_stay_final(monkeypatch):
    """mgdp_vi_synchronize (bench.py's end of the timed region): a resident server leaves at once,
    the stream drains, V / pi of the last served solve are in HBM, and the next solve relaunches."""
    monkeypatch.setenv("MGDP_PERSISTENT", "1")
    monkeypatch.setenv("MGDP_SERVE_IDLE_US", "2000000")  # it would not leave on its own
    t = load("table_empty16_s0.npz")
    cells = cells_from_enc(t["enc"])[None]
    o = oracle.value_iteration(0, cells, dtype="f32")
    vi = mg.ValueIteration(cells, dtype="f32")
    assert vi.persistent and vi.kernel_name == "vi_serve_kernel"
    vi.enable_timing(True)
    for _ in range(5):
        assert vi.solve() == o["sweeps"]
    vi.synchronize()
    ms, n = vi.kernel_time()
    assert n == 1 and ms > 0  # one launch served all five, and it has ended
    np.testing.assert_array_equal(vi.values(), o["V"])
    np.testing.assert_array_equal(vi.policy(), o["pi"])
    assert vi.solve() == o["sweeps"]  # relaunched
    vi.synchronize()
    np.testing.assert_array_equal(vi.values(), o["V"])
    vi.close()
    names = {m: mg.ValueIteration(np.repeat(cells, 2, axis=0), dtype="f32", method=m) for m in ("fused", "sweep")}
    assert names["fused"].kernel_name == "vi_fused_kernel"
    assert names["sweep"].kernel_name == "vi_sweep_pipe_kernel"  # Empty-16: the register-pipelined sweep
    for v in names.values():
        v.close()


def test_persistent_server_lifetime_cap_relaunch(monkeypatch):
    """Servers that leave on their lifetime cap while the host still counts them resident: the
    host finds the stream drained with its request unserved and relaunches; results stay exact."""
    monkeypatch.setenv("MGDP_PERSISTENT", "1")
    monkeypatch.setenv("MGDP_SERVE_LIFE_US", "300")
    t = load("table_lava11n5_s0.npz")
    cells = cells_from_enc(t["enc"])[None]
    o = oracle.value_iteration(0, cells, dtype="f32")
    vi = mg.ValueIteration(cells, dtype="f32")
    assert vi.persistent
    vi.enable_timing(True)
    for _ in range(200):
        assert vi.solve() == o["sweeps"]
    ms, n = vi.kernel_time()
    assert n > 1  # the cap ended several servers
    np.testing.assert_array_equal(vi.values(), o["V"])
    np.testing.assert_array_equal(vi.policy(), o["pi"])
    vi.close()


@pytest.mark.parametrize("persistent", ["0", "1"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("one_tile", ["0", "1"])
def test_fused_doorkey_lone_and_batched_bit_exact(persistent, dtype, one_tile, monkeypatch):
    """DoorKey fused local loop, lone (persistent server or one launch) and batched (two LDS tiles,
    or one tile with two barriers per sweep: MGDP_DK_1T, fp32 batches), including max_sweeps caps
    that end the loop before convergence."""
    monkeypatch.setenv("MGDP_PERSISTENT", persistent)
    monkeypatch.setenv("MGDP_DK_1T", one_tile)
    for env in ("doorkey8", "doorkey16"):
        g = load(f"grids_{env}.npz")
        cells = np.stack([cells_from_enc(e) for e in g["enc"]])
        for sub in (cells[:1], cells[:7], cells):
            r = gpu_vi(sub, "doorkey", dtype, "fused", "cell")
            o = oracle.value_iteration(1, sub, dtype=dtype)
            assert r.sweeps == o["sweeps"]
            np.testing.assert_array_equal(r.V, o["V"])
            np.testing.assert_array_equal(r.pi, o["pi"])
        for ms in (1, 2, 17):
            r = gpu_vi(cells[:3], "doorkey", dtype, "fused", "cell", max_sweeps=ms)
            o = oracle.value_iteration(1, cells[:3], dtype=dtype, max_sweeps=ms)
            assert r.sweeps == o["sweeps"] == ms
            np.testing.assert_array_equal(r.V, o["V"])
            np.testing.assert_array_equal(r.pi, o["pi"])


def test_dk_1t_run_to_continues_resumed_grids(monkeypatch):
    """The one-tile DoorKey loop's run-to instantiation on grids resumed from HBM (the solves above end at
    exact fixed points, which need no second launch): a fresh run_to(5), then on to the oracle's K; the
    sweep count, dV, V and pi bit for bit."""
    monkeypatch.setenv("MGDP_DK_1T", "1")
    cells = np.stack([cells_from_enc(e) for e in load("grids_doorkey16.npz")["enc"][:3]])
    o = oracle.value_iteration(1, cells, dtype="f32")
    vi = mg.ValueIteration(cells, model="doorkey", dtype="f32")
    try:
        assert vi.variant == "dk_1t"
        vi.reset()
        vi.run_to(5)
        dv = vi.run_to(o["sweeps"])
        vi.finish(o["sweeps"], dv)
        assert vi.sweeps == o["sweeps"] and dv == o["dv"]
        np.testing.assert_array_equal(vi.values(), o["V"])
        np.testing.assert_array_equal(vi.policy(), o["pi"])
    finally:
        vi.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_tolerance_threshold_edges(dtype):
    """The kernels test |dV| >= tol against tol rounded up to the value type; exact for tolerances
    that are (2^-20) and are not (1e-6, 3e-7, 0.01) representable in it."""
    g = load("grids_lava11n5.npz")
    cells = np.stack([cells_from_enc(e) for e in g["enc"][:7]])
    for tol in (2.0 ** -20, 1e-6, 3e-7, 0.01):
        for sub in (cells[:1], cells):
            for method in ("fused", "sweep"):
                r = gpu_vi(sub, "xyd", dtype, method, "cell", slip=0.9, tol=tol)
                o = oracle.value_iteration(0, sub, slip_p=0.9, dtype=dtype, tol=tol)
                assert r.sweeps == o["sweeps"]
                np.testing.assert_array_equal(r.V, o["V"])


def _random_xyd_grid(rng, W, H):
    """Closed-border grid with random walls / lava / floor and one goal (XYD cell types)."""
    c = rng.choice(np.array([1, 1, 1, 1, 1, 2, 3, 9], np.uint8), size=(H, W))
    c[0, :] = c[-1, :] = 2
    c[:, 0] = c[:, -1] = 2
    c[rng.integers(1, H - 1), rng.integers(1, W - 1)] = 8
    return c


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_wave_lone_grid_sizes(dtype, monkeypatch):
    """Lone XYD grids of <= 512 cells run on one wave with P = 1, 2, 4, 8 cells per lane
    (fused_wave_xyd): bit-exact vs the oracle and vs the multi-wave loop (MGDP_WAVE=0) at sizes
    on both sides of every P boundary, with slip, max_sweeps caps, one-sweep-at-a-time
    continuation (k > 0 restarts from V in HBM) and the persistent server."""
    rng = np.random.default_rng(7)
    sizes = [(5, 5), (8, 8), (9, 8), (11, 11), (16, 8), (16, 16), (17, 16), (19, 19), (22, 22), (23, 23)]
    for W, H in sizes:
        cells = _random_xyd_grid(rng, W, H)[None]
        for slip in (None, 0.9):
            o = oracle.value_iteration(0, cells, slip_p=slip, dtype=dtype)
            got = {}
            for wave, pers in (("8", "1"), ("8", "0"), ("0", "1"), ("1", "1")):
                monkeypatch.setenv("MGDP_WAVE", wave)
                monkeypatch.setenv("MGDP_PERSISTENT", pers)
                r = gpu_vi(cells, "xyd", dtype, "fused", "cell", slip=slip)
                assert r.sweeps == o["sweeps"], (W, H, slip, wave, pers)
                np.testing.assert_array_equal(r.V, o["V"])
                np.testing.assert_array_equal(r.pi, o["pi"])
                got[(wave, pers)] = r
        monkeypatch.setenv("MGDP_WAVE", "8")
        for pers in ("0", "1"):
            monkeypatch.setenv("MGDP_PERSISTENT", pers)
            for ms in (1, 2, 5):
                r = gpu_vi(cells, "xyd", dtype, "fused", "cell", max_sweeps=ms)
                o = oracle.value_iteration(0, cells, dtype=dtype, max_sweeps=ms)
                assert r.sweeps == o["sweeps"]
                np.testing.assert_array_equal(r.V, o["V"])
                np.testing.assert_array_equal(r.pi, o["pi"])
        vi = mg.ValueIteration(cells, dtype=dtype)
        vi.reset()
        vi.run_to(1)  # fresh, non-local loop to k = 1
        vi.sweep()    # continuations: k = 1 -> 2 -> 3 from V in HBM
        vi.sweep()
        vi.finish(3, 0.0)
        o = oracle.value_iteration(0, cells, dtype=dtype, max_sweeps=3)
        np.testing.assert_array_equal(vi.values(), o["V"])
        np.testing.assert_array_equal(vi.policy(), o["pi"])
        vi.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_maximum_and_ragged_grid_sizes(dtype, monkeypatch):
    """The largest grids the LDS-resident kernels take (32 x 32 = 1024 cells: one thread per cell,
    or 512 threads at two cells per thread) and non-square ones, lone and batched, every XYD
    method against the oracle bit for bit; DoorKey at 32 x 32 in fp32 (two 64 KB V tiles) and the
    refusal of the fp64 one, which cannot fit LDS."""
    rng = np.random.default_rng(11)
    for W, H in ((32, 32), (32, 7), (5, 32), (31, 29)):
        cells = np.stack([_random_xyd_grid(rng, W, H) for _ in range(3)])
        for sub in (cells[:1], cells):
            o = oracle.value_iteration(0, sub, dtype=dtype)
            for method, cpt in (("fused", "1"), ("fused", "2"), ("sweep", "1")):
                monkeypatch.setenv("MGDP_CPT", cpt)
                r = gpu_vi(sub, "xyd", dtype, method, "cell")
                assert r.sweeps == o["sweeps"], (W, H, method, cpt)
                np.testing.assert_array_equal(r.V, o["V"])
                np.testing.assert_array_equal(r.pi, o["pi"])
    from minigrid_dynamicprogramming_amd.envs import DoorKeyEnv

    env = DoorKeyEnv(size=32)
    dk = np.stack([env.generate(seed=s)[0][..., 0].T for s in range(3)]).astype(np.uint8)
    if dtype == "f32":
        for sub in (dk[:1], dk):
            o = oracle.value_iteration(1, sub, dtype="f32")
            r = gpu_vi(sub, "doorkey", "f32", "fused", "cell")
            assert r.sweeps == o["sweeps"]
            np.testing.assert_array_equal(r.V, o["V"])
            np.testing.assert_array_equal(r.pi, o["pi"])
    else:
        with pytest.raises(ValueError):
            gpu_vi(dk[:1], "doorkey", "f64", "fused", "cell")


@pytest.mark.parametrize("pipe", ["0", "1", "2", "3", "4"])
def test_sweep_method_pipeline_depths(pipe, monkeypatch):
    """The per-sweep HBM method on the staged kernel (MGDP_SWEEP_PIPE=0) and on the register-
    pipelined kernel with grids fetched 1-4 strides ahead: every depth bit-exact vs the oracle,
    batches that do not divide the grid-stride (tail handling) included."""
    monkeypatch.setenv("MGDP_SWEEP_PIPE", pipe)
    for env in ("fourrooms", "lava11n5"):
        g = load(f"grids_{env}.npz")
        cells = np.stack([cells_from_enc(e) for e in g["enc"]])
        for sub in (cells[:1], cells[:5], cells):
            for dtype in ("f32", "f64"):
                r = gpu_vi(sub, "xyd", dtype, "sweep", "cell")
                o = oracle.value_iteration(0, sub, dtype=dtype)
                assert r.sweeps == o["sweeps"]
                np.testing.assert_array_equal(r.V, o["V"])
                np.testing.assert_array_equal(r.pi, o["pi"])
