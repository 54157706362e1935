"""The CPU oracle's orc_step_held / orc_gen_obs on cluttered rooms, pinned to the reference's own
rollouts (tests/golden/clutter_v*.npz, make_golden_clutter.py): open and walled rooms from 3x3 to
23x5 holding doors of every colour and state, keys, balls, boxes with contents, floor tiles, lava
and goals, at view sizes 3, 5 and 7, with the front cell outside the grid and unknown actions among
the steps.  tests/test_gpu_clutter.py holds the HIP engine to the same fixtures and, at batch scale,
to this oracle, so the oracle has to stand on the reference here first."""
import os

import numpy as np
import pytest

from tests import clutter_util as cu
from tests.golden_util import GOLDEN

SHAPES = [(3, 3), (4, 3), (5, 4), (6, 7), (7, 5), (9, 6), (11, 9), (13, 10), (17, 3), (3, 12), (10, 10), (23, 5)]


def test_fixture_set_is_complete():
    """24 envs per view size: the twelve shapes x see_through_walls, every third shape walled, one
    env in four with max_steps 60, 128 steps each; no file larger than the largest older fixture."""
    assert cu.fixture_files(), "no clutter fixtures"
    for view in cu.VIEWS:
        envs = cu.load_envs(view)
        assert [(int(e["width"]), int(e["height"]), int(e["see_through"])) for e in envs] == \
            [(w, h, s) for w, h in SHAPES for s in (0, 1)]
        assert all(int(e["view"]) == view and e["actions"].shape == (128,) for e in envs)
        assert [int(e["border"]) for e in envs] == [int(i % 3 == 2) for i in range(12) for _ in (0, 1)]
        short = [e for e in envs if int(e["max_steps"]) == 60]
        assert len(short) == 6 and all(int(e["max_steps"]) == 4 * int(e["width"]) * int(e["height"])
                                       for e in envs if e not in short)
    others = [os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
              if f.endswith(".npz") and not f.startswith("clutter_")]
    for f in cu.fixture_files():
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= max(others), f


@pytest.mark.parametrize("name", cu.fixture_files())
def test_fixture_event_counts(name):
    """Each file holds at least 3 steps of every event class and at most 10 % BOUNDS steps; the
    recorded status agrees with the event bits, and a BOUNDS step leaves an agent whose front cell
    is inside the grid."""
    envs = cu.load_file(name)
    ev = np.stack([e["event"] for e in envs])
    st = np.stack([e["status"] for e in envs])
    counts = cu.count_events(ev)
    assert all(c >= cu.MIN_EVENTS for c in counts.values()), counts
    assert counts["bounds"] <= cu.MAX_BOUNDS_SHARE * ev.size, counts
    np.testing.assert_array_equal((ev & cu.EV["bounds"]) != 0, st == cu.E_BOUNDS)
    np.testing.assert_array_equal((ev & cu.EV["bad_action"]) != 0, st == cu.E_ACTION)
    for e in envs:
        W, H = int(e["width"]), int(e["height"])
        ag = e["agent"].astype(np.int32)
        before = np.concatenate([e["init_agent"][None].astype(np.int32), ag[:-1]])
        bounds = e["status"] == cu.E_BOUNDS
        np.testing.assert_array_equal(cu.reaim(before[bounds], W, H), ag[bounds])  # the re-aim rule
        assert (cu.reaim(before[bounds], W, H)[:, 2] != before[bounds][:, 2]).all()
        trunc = (e["event"] & cu.EV["truncated"]) != 0
        np.testing.assert_array_equal(trunc, (e["truncated"] != 0) & (e["status"] == 0))
        assert (e["image"][e["status"] != 0] == 0).all()


@pytest.mark.parametrize("view", cu.VIEWS)
@pytest.mark.parametrize("stepper", [cu.OracleEnvStepper, cu.OracleBatchStepper], ids=["OracleEnv", "OracleBatch"])
def test_oracle_replays_reference(stepper, view):
    for envs in cu.by_shape(cu.load_envs(view)).values():
        s = stepper(**cu.stack_envs(envs))
        if stepper is cu.OracleEnvStepper:
            for e, o in zip(envs, s.envs):  # gen_obs before any step
                np.testing.assert_array_equal(o.obs(), e["init_image"])
        cu.replay(s, envs, what=stepper.__name__)


def test_events_of_matches_the_fixture_events():
    """clutter_util.events_of (the GPU fuzz's tally) classifies the fixture's steps exactly as the
    generator did from the reference's objects."""
    for view in cu.VIEWS:
        for envs in cu.by_shape(cu.load_envs(view)).values():
            s = cu.OracleBatchStepper(**cu.stack_envs(envs))
            for i in range(128):
                a = np.array([e["actions"][i] for e in envs], np.int32)
                np.testing.assert_array_equal(cu.events_of(s.ob, a), [int(e["event"][i]) for e in envs])
                s.step(a)
                bounds = np.array([e["status"][i] for e in envs]) == cu.E_BOUNDS
                s.set_agent(np.stack([e["agent"][i] for e in envs]).astype(np.int32), bounds)


@pytest.mark.parametrize("W,H,border", [(3, 3, False), (6, 5, True), (23, 5, False)])
def test_random_clutter_rooms(W, H, border):
    """The numpy generator: valid encodings only, contents only in boxes, a wall rim when asked, the
    agent on an empty cell, and every object kind present over the batch."""
    B = 512
    enc, held, agent = cu.random_clutter(B, W, H, seed=3, border=border)
    assert enc.shape == held.shape == (B, W, H, 3) and agent.shape == (B, 3)
    ty, co, st = enc[..., 0], enc[..., 1], enc[..., 2]
    assert ty.min() >= cu.T_EMPTY and ty.max() <= cu.T_LAVA and co.max() <= 5
    assert (st[ty != cu.T_DOOR] == 0).all() and st.max() <= 2
    assert (held[..., 0][ty != cu.T_BOX] == 0).all() and set(np.unique(held[..., 0])) <= {0, 5, 6, 7}
    rows = np.arange(B)
    assert (ty[rows, agent[:, 0], agent[:, 1]] == cu.T_EMPTY).all()
    assert (agent[:, 2] >= 0).all() and (agent[:, 2] < 4).all()
    if border:
        rim = np.ones((W, H), bool)
        rim[1:-1, 1:-1] = False
        assert (ty[:, rim] == cu.T_WALL).all()
    assert set(np.unique(ty)) == set(range(1, 10))
    assert {(4, s) for s in range(3)} <= {(int(t), int(s)) for t, s in zip(ty.ravel(), st.ravel())}
