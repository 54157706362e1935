"""Shared by tests/test_clutter_cpu.py and tests/test_gpu_clutter.py: the cluttered-room fixtures of
tests/golden/make_golden_clutter.py (clutter_v*.npz), a numpy generator of rooms of the same object
mix, the re-aim rule for an agent that faces out of an open grid, the event classes of a step, and
the replay loop that holds a stepper (the oracle, or the HIP engine) to a fixture."""
import glob
import os

import numpy as np

from oracle import oracle
from tests.golden_util import GOLDEN

E_ACTION, E_BOUNDS = -4, -5  # MGDP_E_ACTION, MGDP_E_BOUNDS (include/mgdp.h)
VIEWS = (3, 5, 7)
EVENTS = ("unlock", "wrong_key", "no_key", "door_flip", "enter_door", "pickup", "pickup_refused", "drop",
          "box_full", "box_empty", "goal", "lava", "truncated", "bounds", "bad_action")
EV = {n: 1 << i for i, n in enumerate(EVENTS)}
MIN_EVENTS, MAX_BOUNDS_SHARE = 3, 0.10  # per fixture file (make_golden_clutter.py asserts the same)
DX = np.array([1, 0, -1, 0])
DY = np.array([0, 1, 0, -1])
T_EMPTY, T_WALL, T_FLOOR, T_DOOR, T_KEY, T_BALL, T_BOX, T_GOAL, T_LAVA = 1, 2, 3, 4, 5, 6, 7, 8, 9
D_OPEN, D_CLOSED, D_LOCKED = 0, 1, 2


def fixture_files(view=None):
    pat = "clutter_v*.npz" if view is None else f"clutter_v{view}*.npz"
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, pat)))


_CACHE = {}


def load_file(name):
    """One fixture file as a list of per-env dicts (grids reshaped to (W, H, 3)); read once."""
    if name not in _CACHE:
        t = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
        envs = []
        for i in range(len(t["width"])):
            W, H = int(t["width"][i]), int(t["height"][i])
            e = {k: t[k][i] for k in t.files if k != "enc_off" and t[k].shape[:1] == t["width"].shape
                 and k not in ("init_enc", "init_held", "final_enc", "final_held")}
            lo, hi = t["enc_off"][i], t["enc_off"][i + 1]
            for k in ("init_enc", "init_held", "final_enc", "final_held"):
                e[k] = t[k][lo:hi].reshape(W, H, 3)
            e["file"] = name
            for k, v in e.items():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            envs.append(e)
        _CACHE[name] = envs
    return _CACHE[name]


def load_envs(view):
    """The 24 fixture envs of one agent_view_size, in shape order."""
    envs = [e for f in fixture_files(view) for e in load_file(f)]
    return sorted(envs, key=lambda e: (int(e["seed"])))


def by_shape(envs):
    """Fixture envs grouped by (W, H): each group steps on one handle / one OracleBatch."""
    groups = {}
    for e in envs:
        groups.setdefault((int(e["width"]), int(e["height"])), []).append(e)
    return groups


def reaim(agent, W, H):
    """The re-aim rule: an agent whose front cell is outside the grid can never move again (turns
    assert too), so it is turned clockwise until the cell in front of it is inside.  agent (B, 3)."""
    agent = np.array(agent, np.int32)
    for _ in range(3):
        fx, fy = agent[:, 0] + DX[agent[:, 2]], agent[:, 1] + DY[agent[:, 2]]
        out = (fx < 0) | (fy < 0) | (fx >= W) | (fy >= H)
        agent[out, 2] = (agent[out, 2] + 1) & 3
    return agent


def random_clutter(B, W, H, seed, border):
    """B rooms of the fixture rooms' object mix in plain numpy: enc, held (B, W, H, 3) x-major
    encodings and agent (B, 3).  About 45 % of the cells (inside the wall border, if any) hold a
    wall or floor tile of any colour, a door of any colour and state, a key, a ball, a box (holding
    nothing, a key, a ball or a box), lava or a goal; the agent stands on an emptied cell, on the
    rim too when there is no border, heading anywhere."""
    rng = np.random.default_rng(seed)
    kinds = np.array([T_WALL] * 5 + [T_FLOOR] * 5 + [T_DOOR] * 6 + [T_KEY] * 4 + [T_BALL] * 3 + [T_BOX] * 6
                     + [T_LAVA] * 2 + [T_GOAL] * 2, np.uint8)
    shape = (B, W, H)
    ty = kinds[rng.integers(0, len(kinds), shape)]
    co = rng.integers(0, 6, shape).astype(np.uint8)
    co = np.where(ty == T_GOAL, 1, np.where(ty == T_LAVA, 0, co))
    st = np.where(ty == T_DOOR, rng.integers(0, 3, shape), 0).astype(np.uint8)
    hty = np.array([0, T_KEY, T_BALL, T_BOX], np.uint8)[rng.integers(0, 4, shape)]
    hco = rng.integers(0, 6, shape).astype(np.uint8)
    filled = rng.random(shape) < 0.45
    b = 1 if border else 0
    ax, ay = rng.integers(b, W - b, B), rng.integers(b, H - b, B)
    filled[np.arange(B), ax, ay] = False
    enc = np.zeros((B, W, H, 3), np.uint8)
    enc[..., 0] = np.where(filled, ty, T_EMPTY)
    enc[..., 1] = np.where(filled, co, 0)
    enc[..., 2] = np.where(filled, st, 0)
    if border:
        for sl in ((slice(None), 0), (slice(None), H - 1), (0, slice(None)), (W - 1, slice(None))):
            enc[(slice(None),) + sl] = (T_WALL, 5, 0)
    held = np.zeros_like(enc)
    box = (enc[..., 0] == T_BOX) & (hty > 0)
    held[..., 0] = np.where(box, hty, 0)
    held[..., 1] = np.where(box, hco, 0)
    agent = np.stack([ax, ay, rng.integers(0, 4, B)], axis=1).astype(np.int32)
    return enc, held, agent


def batch_enc(ob):
    """An OracleBatch's grids as (B, W, H, 3) x-major encodings."""
    B, W, H = ob.B, ob.W, ob.H
    return np.stack([q[:, : W * H].reshape(B, H, W).transpose(0, 2, 1) for q in (ob.ty, ob.co, ob.st)], axis=-1)


def events_of(ob, actions):
    """(B,) event bit sets of the step an OracleBatch is about to take with `actions`."""
    B, W, H = ob.B, ob.W, ob.H
    a = np.asarray(actions)
    x, y, d, sc = ob.state.T
    fx, fy = x + DX[d], y + DY[d]
    inb = (fx >= 0) & (fy >= 0) & (fx < W) & (fy < H)
    fi = np.where(inb, fy * W + fx, 0)
    rows = np.arange(B)
    ft, fc, fs = ob.ty[rows, fi], ob.co[rows, fi], ob.st[rows, fi]
    fh = ob.hty[rows, fi] if ob.hty is not None else np.zeros(B, np.uint8)
    ct, cc = ob.carry.T
    act_ok = (a >= 0) & (a <= 6)
    ok = inb & act_ok
    door, locked = ft == T_DOOR, (ft == T_DOOR) & (fs == D_LOCKED)
    key = ct == T_KEY
    can_pickup = (ft == T_KEY) | (ft == T_BALL) | (ft == T_BOX)
    parts = {
        "bounds": ~inb,
        "bad_action": inb & ~act_ok,
        "truncated": ok & (sc + 1 >= ob.max_steps),
        "drop": ok & (a == 4) & (ft == T_EMPTY) & (ct != 0),
        "goal": ok & (a == 2) & (ft == T_GOAL),
        "lava": ok & (a == 2) & (ft == T_LAVA),
        "enter_door": ok & (a == 2) & door & (fs == D_OPEN),
        "pickup": ok & (a == 3) & can_pickup & (ct == 0),
        "pickup_refused": ok & (a == 3) & can_pickup & (ct != 0),
        "door_flip": ok & (a == 5) & door & ~locked,
        "no_key": ok & (a == 5) & locked & ~key,
        "unlock": ok & (a == 5) & locked & key & (cc == fc),
        "wrong_key": ok & (a == 5) & locked & key & (cc != fc),
        "box_full": ok & (a == 5) & (ft == T_BOX) & (fh > T_EMPTY),
        "box_empty": ok & (a == 5) & (ft == T_BOX) & (fh <= T_EMPTY),
    }
    ev = np.zeros(B, np.int64)
    for n, m in parts.items():
        ev |= np.where(m, EV[n], 0)
    return ev


def count_events(ev):
    ev = np.asarray(ev).astype(np.int64)
    return {n: int(((ev & EV[n]) != 0).sum()) for n in EVENTS}


# ---------------------------------------------------------------------------------------- steppers
# A stepper steps a batch of envs of one shape.  step(actions) -> dict(image, direction, reward,
# terminated, truncated, status) with status in MGDP codes; set_agent(agent (B, 3), mask (B,));
# state(grids) -> dict(agent, carry, carry_held, step_count[, enc, held]).
_ORC_STATUS = {0: 0, -1: E_ACTION, -2: E_BOUNDS}  # orc_step_held's return codes


class OracleBatchStepper:
    def __init__(self, enc, held, agent, max_steps, see_through, view):
        self.ob = oracle.OracleBatch(enc, agent, max_steps, see_through, view=view, held=held)

    def step(self, actions):
        ob = self.ob
        ob.step(np.asarray(actions, np.int32))
        status = np.array([_ORC_STATUS[int(s)] for s in ob.status], np.int32)
        return dict(image=ob.obs.copy(), direction=ob.state[:, 2].copy(), reward=ob.reward.copy(),
                    terminated=ob.terminated.copy(), truncated=ob.truncated.copy(), status=status)

    def set_agent(self, agent, mask):
        m = np.asarray(mask, bool)
        self.ob.state[m, :3] = np.asarray(agent, np.int32)[m]

    def set_carry(self, carry, mask):
        m = np.asarray(mask, bool)
        self.ob.carry[m] = np.asarray(carry, np.int32)[m]
        self.ob.held_carry[m] = 0  # a new carry holds nothing

    def state(self, grids=False):
        ob = self.ob
        st = dict(agent=ob.state[:, :3].copy(), step_count=ob.state[:, 3].copy(), carry=ob.carry.copy(),
                  carry_held=ob.held_carry.copy())
        if grids:
            st["enc"], st["held"] = batch_enc(ob), ob.held_encoding()
        return st


class OracleEnvStepper:
    """The same interface over one OracleEnv per env (orc_step_held called env by env)."""

    def __init__(self, enc, held, agent, max_steps, see_through, view):
        self.envs = [oracle.OracleEnv(enc[i], agent[i], int(max_steps[i]), bool(see_through[i]), view=view, held=held[i])
                     for i in range(len(enc))]
        self.view = view

    def step(self, actions):
        B, v = len(self.envs), self.view
        out = dict(image=np.zeros((B, v, v, 3), np.uint8), direction=np.zeros(B, np.int32), reward=np.zeros(B),
                   terminated=np.zeros(B, np.uint8), truncated=np.zeros(B, np.uint8), status=np.zeros(B, np.int32))
        for i, (e, a) in enumerate(zip(self.envs, actions)):
            try:
                out["image"][i], out["reward"][i], out["terminated"][i], out["truncated"][i] = e.step(int(a))
            except ValueError:
                out["status"][i] = E_ACTION
            except AssertionError:
                out["status"][i] = E_BOUNDS
            out["direction"][i] = e.state[2]
        return out

    def set_agent(self, agent, mask):
        for i, e in enumerate(self.envs):
            if mask[i]:
                e.state[:3] = agent[i]

    def state(self, grids=False):
        es = self.envs
        st = dict(agent=np.stack([e.state[:3] for e in es]), step_count=np.array([e.state[3] for e in es]),
                  carry=np.stack([e.carry for e in es]), carry_held=np.stack([e.held_carry for e in es]))
        if grids:
            st["enc"] = np.stack([e.encode() for e in es])
            st["held"] = np.stack([e.held_encoding() for e in es])
        return st


def stack_envs(envs):
    """Constructor arguments of a stepper for fixture envs of one shape and view."""
    return dict(enc=np.stack([e["init_enc"] for e in envs]), held=np.stack([e["init_held"] for e in envs]),
                agent=np.stack([e["init_agent"] for e in envs]).astype(np.int32),
                max_steps=np.array([e["max_steps"] for e in envs], np.int32),
                see_through=np.array([e["see_through"] for e in envs], np.uint8), view=int(envs[0]["view"]))


def replay(stepper, envs, what=""):
    """Step `stepper` (built from stack_envs(envs)) through the fixture envs' recorded actions and
    hold every step to the reference's record: status, agent, step_count, carry and carried contents
    on every step; image, direction, reward and flags where the reference did not raise; after a
    BOUNDS step the recorded (re-aimed) agent is applied, as the generator did; the final grids and
    Box contents."""
    eq = np.testing.assert_array_equal
    rec = {k: np.stack([e[k] for e in envs]) for k in ("actions", "image", "direction", "reward", "terminated",
                                                       "truncated", "status", "agent", "carry", "carry_held",
                                                       "step_count")}
    for i in range(rec["actions"].shape[1]):
        ctx = f"{what} {envs[0]['file']} {int(envs[0]['width'])}x{int(envs[0]['height'])} step {i}"
        out = stepper.step(rec["actions"][:, i].astype(np.int32))
        eq(out["status"], rec["status"][:, i], err_msg=ctx)
        ok = rec["status"][:, i] == 0
        eq(out["image"][ok], rec["image"][:, i][ok], err_msg=ctx)
        for k in ("direction", "reward", "terminated", "truncated"):
            eq(np.asarray(out[k])[ok], rec[k][:, i][ok], err_msg=f"{ctx} {k}")
        bounds = rec["status"][:, i] == E_BOUNDS
        if bounds.any():
            stepper.set_agent(rec["agent"][:, i].astype(np.int32), bounds)
        st = stepper.state()
        for k in ("agent", "step_count", "carry", "carry_held"):
            eq(st[k], rec[k][:, i], err_msg=f"{ctx} {k}")
    st = stepper.state(grids=True)
    eq(st["enc"], np.stack([e["final_enc"] for e in envs]), err_msg=f"{what} final grids")
    eq(st["held"], np.stack([e["final_held"] for e in envs]), err_msg=f"{what} final contents")


# ---------------------------------------------------------------------------------------- the fuzz
FUZZ_B, FUZZ_STEPS = 1029, 48  # 4 * 256 + 5 envs: a partial last workgroup at every group size
# (W, H, border, views, all_groups): open and walled grids alternate, the view sizes rotate
FUZZ_SHAPES = [(3, 3), (4, 4), (5, 4), (6, 7), (7, 5), (8, 6), (9, 6), (13, 10), (16, 3), (3, 16), (23, 5), (33, 31),
               (40, 30)]
FUZZ_ALL_VIEWS = {(5, 4), (9, 6), (33, 31)}
FUZZ_ALL_GROUPS = {(4, 4), (13, 10), (40, 30)}


def fuzz_cases():
    """(W, H, border, view, group) of every fuzz run; group None = the engine's default."""
    cases = []
    for i, (W, H) in enumerate(FUZZ_SHAPES):
        views = VIEWS if (W, H) in FUZZ_ALL_VIEWS else (VIEWS[i % 3],)
        groups = ("1", "2", "4", "8") if (W, H) in FUZZ_ALL_GROUPS else (None,)
        cases += [(W, H, i % 2 == 1, v, g) for v in views for g in groups]
    return cases


def fuzz_actions(rng, B):
    """Left / right / forward / pickup / drop / toggle / done, and -1, 7, 100 at 1 % together."""
    p = np.array([0.10, 0.10, 0.27, 0.15, 0.12, 0.21, 0.04, 0.01])
    a = rng.choice(8, size=B, p=p).astype(np.int32)
    bad = a == 7
    a[bad] = np.array([-1, 7, 100], np.int32)[rng.integers(0, 3, int(bad.sum()))]
    return a


def expected_events(border):
    return set(EVENTS) - ({"bounds"} if border else set())


def fuzz(W, H, border, view, make_stepper=None, seed=0, B=FUZZ_B, steps=FUZZ_STEPS):
    """Random actions on B random_clutter rooms with per-env see_through and max_steps in [1, 80].
    An env that starts in front of a locked door carries a key, of the door's colour in every other
    such env, and toggles first, so unlocking and the wrong-colour refusal happen in every run.
    After a BOUNDS step the agent is re-aimed (reaim) on both sides.  make_stepper(...) builds the
    stepper under test, which is held to the OracleBatch on every step (image where status is 0,
    reward, flags, direction, status) and, every 8 steps and at the end, in agent, carry, carried
    contents, step_count, grids and Box contents; None runs the oracle alone.  Returns the event
    counts of the run."""
    eq = np.testing.assert_array_equal
    enc, held, agent = random_clutter(B, W, H, seed, border)
    rng = np.random.default_rng(seed + 1)
    see = rng.integers(0, 2, B).astype(np.uint8)
    ms = rng.integers(1, 81, B).astype(np.int32)
    args = dict(enc=enc, held=held, agent=agent, max_steps=ms, see_through=see, view=view)
    ref = OracleBatchStepper(**args)
    dut = make_stepper(**args) if make_stepper else None
    fx, fy = agent[:, 0] + DX[agent[:, 2]], agent[:, 1] + DY[agent[:, 2]]
    inb = (fx >= 0) & (fy >= 0) & (fx < W) & (fy < H)
    front = enc[np.arange(B), np.where(inb, fx, 0), np.where(inb, fy, 0)]
    locked = inb & (front[:, 0] == T_DOOR) & (front[:, 2] == D_LOCKED)
    carry = np.zeros((B, 2), np.int32)
    nth = np.cumsum(locked) - 1
    carry[locked] = np.stack([np.full(int(locked.sum()), T_KEY), (front[locked, 1] + nth[locked] % 2) % 6], axis=1)
    for s in (ref, dut) if dut else (ref,):
        s.set_carry(carry, locked)
    total = np.zeros(len(EVENTS), np.int64)
    for t in range(steps):
        a = fuzz_actions(rng, B)
        if t == 0:
            a[locked] = 5
        ev = events_of(ref.ob, a)
        total += [int(((ev & EV[n]) != 0).sum()) for n in EVENTS]
        want = ref.step(a)
        bounds = want["status"] == E_BOUNDS
        aimed = reaim(ref.ob.state[:, :3], W, H)
        if dut:
            got = dut.step(a)
            ctx = f"{W}x{H} view {view} step {t}"
            eq(got["status"], want["status"], err_msg=ctx)
            ok = want["status"] == 0
            eq(got["image"][ok], want["image"][ok], err_msg=ctx)
            for k in ("reward", "terminated", "truncated", "direction"):
                eq(got[k], want[k], err_msg=f"{ctx} {k}")
            dut.set_agent(aimed, bounds)
        ref.set_agent(aimed, bounds)
        if dut and (t % 8 == 7 or t == steps - 1):
            g, w = dut.state(grids=True), ref.state(grids=True)
            for k in w:
                eq(g[k], w[k], err_msg=f"{W}x{H} view {view} after step {t}: {k}")
    return dict(zip(EVENTS, total.tolist()))
