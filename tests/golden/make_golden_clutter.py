"""Golden trajectories on cluttered rooms of every object type, from the reference itself.

Runs only where a checkout of the reference (Minigrid 2.3.1) is at hand; it is imported through the
offline gymnasium/pygame stand-in under tests/golden/shim, like make_golden_box.py.  The target
families generate walled, mostly square grids with a handful of object kinds; this script builds
ClutterRoom, a MiniGridEnv of the reference's own classes whose grid is W x H (non-square, narrower
than the view, with or without a wall border) and holds walls and floor tiles of every colour, doors
of every colour and state, keys, balls, boxes (holding nothing, a Key, a Ball or a Box), lava and a
rare goal, all drawn from the env's np_random.  Without a border the agent can face out of the grid:
the reference's Grid.get assertion then fires (for turns too, after step_count += 1), and the agent
is stuck, so the script turns it clockwise until its front cell is inside the grid again; every
replay applies the recorded agent the same way.

    PYTHONPATH=tests/golden/shim:<reference checkout> PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_golden_clutter.py

24 envs per agent_view_size (3, 5, 7) = 12 shapes x see_through_walls: clutter_v3.npz, and for views
5 and 7, where one file would pass the size of the largest fixture, one file per see_through value
(clutter_v5_s0.npz, clutter_v5_s1.npz, ...).  Grids of different shapes are stored flat, cut by
enc_off.  Per env width, height, border, see_through,
max_steps, view, seed, init_agent, actions; init_enc / init_held / final_enc / final_held (x-major
(W, H, 3), flattened); init_image; per step image, direction, reward (fp64), terminated, truncated,
status (0, -4 unknown action, -5 front cell outside the grid), agent (after any re-aim), carry,
carry_held, step_count and event (a bit set of EVENTS).  On a failed step the image is zeros and
direction, reward and the flags are not the reference's (it raised): replays skip them."""
from __future__ import annotations

import os

import numpy as np
from minigrid.core.grid import Grid  # noqa: E402  (reference, via the shim)
from minigrid.core.mission import MissionSpace  # noqa: E402
from minigrid.core.world_object import Ball, Box, Door, Floor, Goal, Key, Lava, Wall  # noqa: E402
from minigrid.minigrid_env import MiniGridEnv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
COLORS = ["red", "green", "blue", "purple", "yellow", "grey"]
SHAPES = [(3, 3), (4, 3), (5, 4), (6, 7), (7, 5), (9, 6), (11, 9), (13, 10), (17, 3), (3, 12), (10, 10), (23, 5)]
N_STEPS = 128
DENSITY = 0.45
MAX_BYTES = 22600  # the largest fixture tests/golden held before these
EVENTS = ("unlock", "wrong_key", "no_key", "door_flip", "enter_door", "pickup", "pickup_refused", "drop",
          "box_full", "box_empty", "goal", "lava", "truncated", "bounds", "bad_action")
EV = {n: 1 << i for i, n in enumerate(EVENTS)}
MIN_EVENTS, MAX_BOUNDS_SHARE = 3, 0.10
KINDS = ["wall"] * 5 + ["floor"] * 5 + ["door"] * 6 + ["key"] * 4 + ["ball"] * 3 + ["box"] * 6 + ["lava"] * 2 + ["goal"] * 2
# left, right, forward, pickup, drop, toggle, done, and the unknown action 7
ACTION_P = np.array([0.10, 0.10, 0.26, 0.15, 0.12, 0.21, 0.04, 0.02])
OPENING = [3, 2, 5, 5, 5, 2, 2, 4]  # pickup, forward, toggle (unlock / refuse, close, reopen), through, drop
DXY = [(1, 0), (0, 1), (-1, 0), (0, -1)]


class ClutterRoom(MiniGridEnv):
    def __init__(self, width, height, border, agent_view_size, see_through_walls, max_steps, opening=None):
        self.border, self.opening = border, opening  # opening: None, "match" or "other"
        super().__init__(mission_space=MissionSpace(mission_func=lambda: "wander the clutter"), width=width,
                         height=height, max_steps=max_steps, agent_view_size=agent_view_size,
                         see_through_walls=see_through_walls)

    def _rand_obj(self):
        kind = KINDS[self._rand_int(0, len(KINDS))]
        color = COLORS[self._rand_int(0, len(COLORS))]
        if kind == "wall":
            return Wall(color)
        if kind == "floor":
            return Floor(color)
        if kind == "door":
            state = self._rand_int(0, 3)
            return Door(color, is_open=state == 0, is_locked=state == 2)
        if kind == "key":
            return Key(color)
        if kind == "ball":
            return Ball(color)
        if kind == "box":
            inner = COLORS[self._rand_int(0, len(COLORS))]
            return Box(color, contains=[None, Key(inner), Ball(inner), Box(inner)][self._rand_int(0, 4)])
        return Lava() if kind == "lava" else Goal()

    def _gen_grid(self, width, height):
        self.grid = Grid(width, height)
        b = 1 if self.border else 0
        if b:
            self.grid.wall_rect(0, 0, width, height)
        for x in range(b, width - b):
            for y in range(b, height - b):
                if self._rand_float(0, 1) < DENSITY:
                    self.grid.set(x, y, self._rand_obj())
        if self.opening:  # agent, Key, locked Door and two free cells in a row, heading east
            y = self._rand_int(b, height - b)
            kc = self._rand_int(0, len(COLORS))
            dc = kc if self.opening == "match" else (kc + 1 + self._rand_int(0, len(COLORS) - 1)) % len(COLORS)
            for x in range(b, b + 5):
                self.grid.set(x, y, None)
            self.grid.set(b + 1, y, Key(COLORS[kc]))
            self.grid.set(b + 2, y, Door(COLORS[dc], is_locked=True))
            self.agent_pos, self.agent_dir = (b, y), 0
        else:
            if all(self.grid.get(x, y) is not None for x in range(b, width - b) for y in range(b, height - b)):
                self.grid.set(self._rand_int(b, width - b), self._rand_int(b, height - b), None)
            self.place_agent()
        self.mission = "wander the clutter"


def held_encoding(env):
    out = np.zeros((env.width, env.height, 3), np.uint8)
    for x in range(env.width):
        for y in range(env.height):
            c = env.grid.get(x, y)
            if c is not None and c.type == "box" and c.contains is not None:
                out[x, y] = c.contains.encode()
    return out


def agent_of(env):
    return int(env.agent_pos[0]), int(env.agent_pos[1]), int(env.agent_dir)


def front_inside(env):
    x, y, d = agent_of(env)
    return 0 <= x + DXY[d][0] < env.width and 0 <= y + DXY[d][1] < env.height


def event_of(env, a):
    """What step(a) is about to do, read off the reference's state before the step."""
    x, y, d = agent_of(env)
    if not front_inside(env):
        return EV["bounds"]
    if not 0 <= a <= 6:
        return EV["bad_action"]
    ev = EV["truncated"] if env.step_count + 1 >= env.max_steps else 0
    f = env.grid.get(x + DXY[d][0], y + DXY[d][1])
    c = env.carrying
    if f is None:
        return ev | (EV["drop"] if a == 4 and c is not None else 0)
    if a == 2:
        ev |= {"goal": EV["goal"], "lava": EV["lava"]}.get(f.type, 0)
        ev |= EV["enter_door"] if f.type == "door" and f.is_open else 0
    elif a == 3 and f.can_pickup():
        ev |= EV["pickup"] if c is None else EV["pickup_refused"]
    elif a == 5 and f.type == "door":
        if not f.is_locked:
            ev |= EV["door_flip"]
        elif c is None or c.type != "key":
            ev |= EV["no_key"]
        else:
            ev |= EV["unlock"] if c.color == f.color else EV["wrong_key"]
    elif a == 5 and f.type == "box":
        ev |= EV["box_empty"] if f.contains is None else EV["box_full"]
    return ev


def rollout(view, e, seed0):
    si, see = divmod(e, 2)
    W, H = SHAPES[si]
    opening = None
    if W >= 6:
        k = sum(2 for w, _ in SHAPES[:si] if w >= 6) + see
        opening = ("match", "other", None)[k % 3]
    env = ClutterRoom(W, H, si % 3 == 2, view, bool(see), 60 if (si + 2 * see) % 4 == 1 else 4 * W * H, opening)
    seed = seed0 + e
    obs, _ = env.reset(seed=seed)
    acts = np.random.default_rng(seed0 + 1000 + e).choice(8, size=N_STEPS, p=ACTION_P).astype(np.int32)
    if opening:
        acts[: len(OPENING)] = OPENING
    env_row = dict(width=W, height=H, border=int(env.border), see_through=see, max_steps=env.max_steps, view=view,
                   seed=seed, init_agent=agent_of(env), actions=acts, init_image=obs["image"],
                   init_enc=env.grid.encode().ravel(), init_held=held_encoding(env).ravel())
    keys = ("image", "direction", "reward", "terminated", "truncated", "status", "agent", "carry", "carry_held",
            "step_count", "event")
    rows = {k: [] for k in keys}
    for a in acts:
        rows["event"].append(event_of(env, int(a)))
        d0 = int(env.agent_dir)
        try:
            obs, r, te, tr, _ = env.step(int(a))
            out = (obs["image"], int(obs["direction"]), float(r), bool(te), bool(tr), 0)
        except AssertionError:  # Grid.get: the front cell is outside the grid
            out = (np.zeros((view, view, 3), np.uint8), d0, 0.0, False, False, -5)
            while not front_inside(env):
                env.agent_dir = (env.agent_dir + 1) % 4
        except ValueError:  # unknown action
            out = (np.zeros((view, view, 3), np.uint8), d0, 0.0, False, False, -4)
        for k, v in zip(keys, out):
            rows[k].append(v)
        rows["agent"].append(agent_of(env))
        c = env.carrying
        rows["carry"].append((0, 0) if c is None else tuple(int(v) for v in c.encode()[:2]))
        inner = getattr(c, "contains", None) if c is not None and c.type == "box" else None
        rows["carry_held"].append((0, 0, 0) if inner is None else tuple(int(v) for v in inner.encode()))
        rows["step_count"].append(env.step_count)
    env_row["final_enc"] = env.grid.encode().ravel()
    env_row["final_held"] = held_encoding(env).ravel()
    return env_row, rows


def make(view, seed0, parts):
    """Roll out the 24 envs of one view size and write them as `parts` files (2: one per
    see_through_walls value, where one file would be larger than MAX_BYTES)."""
    flat = ("init_enc", "init_held", "final_enc", "final_held")
    runs = [rollout(view, e, seed0) for e in range(2 * len(SHAPES))]
    for part in range(parts):
        name = f"clutter_v{view}.npz" if parts == 1 else f"clutter_v{view}_s{part}.npz"
        out = {}
        for env_row, rows in runs[part::parts]:
            for k, v in list(env_row.items()) + list(rows.items()):
                out.setdefault(k, []).append(v)
        dt = {"reward": np.float64, "event": np.uint16, "status": np.int8, "direction": np.int8, "agent": np.int8,
              "carry": np.int8, "carry_held": np.int8, "init_agent": np.int8, "actions": np.int8,
              "step_count": np.int16, "image": np.uint8, "init_image": np.uint8, "terminated": np.uint8,
              "truncated": np.uint8}
        arrs = {k: np.concatenate(v).astype(np.uint8) if k in flat else np.array(v, dt.get(k, np.int32))
                for k, v in out.items()}
        arrs["enc_off"] = np.concatenate([[0], np.cumsum([len(v) for v in out["init_enc"]])]).astype(np.int32)
        ev, st = arrs["event"], arrs["status"]
        counts = {n: int(((ev & EV[n]) != 0).sum()) for n in EVENTS}
        share = counts["bounds"] / ev.size
        assert counts["bounds"] == int((st == -5).sum()) and counts["bad_action"] == int((st == -4).sum())
        short = {n: c for n, c in counts.items() if c < MIN_EVENTS}
        assert not short, f"{name}: fewer than {MIN_EVENTS} steps of {short}: change the seed or the density"
        assert share <= MAX_BOUNDS_SHARE, f"{name}: {share:.1%} of the steps are BOUNDS"
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        print(f"{name} {size} bytes, BOUNDS share {share:.1%}, events {counts}", flush=True)
        assert size <= MAX_BYTES, f"{name} is {size} bytes (limit {MAX_BYTES})"


if __name__ == "__main__":
    for view, seed0, parts in ((3, 301, 1), (5, 506, 2), (7, 703, 2)):
        make(view, seed0, parts)
