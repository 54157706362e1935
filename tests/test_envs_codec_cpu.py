"""The env half's cell codec (csrc/envs_codec.h): Grid.encode() layout <-> device planes, Box contents, the
agent check and the masked load's staging layout.

The header is host-plain C++, so it is checked here: tools/envs_codec_check.cpp (its own main, nothing but
envs_codec.h) is built with the host compiler under AddressSanitizer + UBSan and driven through stdin.  The
shapes are the smallest that can go wrong: W=3, H=4 (not square: an x/y transposition moves cells; HW=12 and
HWp=16: padding exists), B=2 with the mask [0, 1] and with none.
"""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "minigrid_dynamicprogramming_amd", "csrc")
B, W, H, HWP = 2, 3, 4, 16
T_EMPTY, T_WALL, T_DOOR, T_KEY, T_BALL, T_BOX, T_AGENT = 1, 2, 4, 5, 6, 7, 10
WALL = T_WALL * 8 + 5  # kCodeWall: a grey wall


def code(t, c, s):
    """The comment above cell_code, written out: type*8 + colour, or 0x80 | state*8 + colour for a door."""
    return (0x80 | s * 8 + c) if t == T_DOOR else t * 8 + c


@pytest.fixture(scope="module")
def codec_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("envs_codec") / "envs_codec_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tools", "envs_codec_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run(exe, cmd, *ints):
    flat = []
    for x in ints:
        flat.extend(x if isinstance(x, (list, tuple)) else [x])
    r = subprocess.run([exe], input=cmd + " " + " ".join(str(int(x)) for x in flat) + "\n", capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = r.stdout.split()
    if out and out[0] in ("ok", "err"):
        return out[0], [int(x) for x in out[1:]]
    return [int(x) for x in out]


def enc_of(cells):
    """cells[b][(x, y)] -> (t, c, s), missing = empty; the flat (B, W, H, 3) array of Grid.encode() layout."""
    flat = []
    for b in range(B):
        for x in range(W):
            for y in range(H):
                flat.extend(cells[b].get((x, y), (T_EMPTY, 0, 0)))
    return flat


def plane_index(b, x, y):
    return b * HWP + y * W + x  # row-major, each env padded to HWp


def stored(tcs):
    """An empty cell carries no colour and no state, whatever was passed in; every other valid cell is kept."""
    return (T_EMPTY, 0, 0) if tcs[0] == T_EMPTY else tcs


VALID = [(t, c, 0) for t in range(11) if t != T_DOOR for c in range(6)] + [(T_DOOR, c, s) for c in range(6) for s in range(3)]


def test_round_trip_is_the_identity_on_every_valid_cell(codec_exe):
    assert len(VALID) == 78
    for k0 in range(0, len(VALID), B * W * H):
        chunk = VALID[k0:k0 + B * W * H]
        cells, want = [{} for _ in range(B)], [WALL] * (B * HWP)
        for k, tcs in enumerate(chunk):
            b, x, y = k // (W * H), (k % (W * H)) // H, k % H
            cells[b][(x, y)] = tcs
        for b in range(B):
            for x in range(W):
                for y in range(H):
                    want[plane_index(b, x, y)] = code(*stored(cells[b].get((x, y), (T_EMPTY, 0, 0))))
        status, plane = run(codec_exe, "encode", B, W, H, HWP, 0, enc_of(cells))
        assert status == "ok" and plane == want
        assert run(codec_exe, "decode", B, W, H, HWP, plane) == enc_of([{k: stored(v) for k, v in c.items()} for c in cells])


def test_empty_decodes_to_colour_and_state_zero_whatever_was_passed(codec_exe):
    cells = [{(2, 1): (T_EMPTY, 3, 2)}, {(0, 3): (T_EMPTY, 200, 77)}]
    status, plane = run(codec_exe, "encode", B, W, H, HWP, 0, enc_of(cells))
    assert status == "ok" and plane[plane_index(0, 2, 1)] == code(T_EMPTY, 0, 0) == plane[plane_index(1, 0, 3)]
    assert run(codec_exe, "decode", B, W, H, HWP, plane) == enc_of([{}, {}])


def test_padding_and_masked_out_envs_hold_the_wall_code(codec_exe):
    cells = [{(0, 0): (11, 9, 9)}, {(1, 2): (T_KEY, 4, 0)}]  # env 0 is masked out: its cells are not looked at
    status, plane = run(codec_exe, "encode", B, W, H, HWP, 1, [0, 1], enc_of(cells))
    assert status == "ok"
    assert plane[:HWP] == [WALL] * HWP
    assert plane[HWP + W * H:] == [WALL] * (HWP - W * H)
    assert plane[plane_index(1, 1, 2)] == code(T_KEY, 4, 0)
    status, plane = run(codec_exe, "encode", B, W, H, HWP, 0, enc_of([{}, cells[1]]))
    assert status == "ok" and plane[W * H:HWP] == [WALL] * (HWP - W * H) == plane[HWP + W * H:]
    assert plane[:W * H] == [code(T_EMPTY, 0, 0)] * (W * H)


@pytest.mark.parametrize("bad", [(11, 0, 0), (T_KEY, 6, 0), (T_BALL, 1, 1), (T_DOOR, 2, 3)],
                         ids=["type11", "colour6", "nondoor_state1", "door_state3"])
def test_invalid_cells_are_refused_with_their_env_and_coordinates(codec_exe, bad):
    for masked, (b, x, y) in ((0, (0, 2, 1)), (1, (1, 1, 3)), (0, (1, 0, 2))):
        cells = [{}, {}]
        cells[b][(x, y)] = bad
        status, err = run(codec_exe, "encode", B, W, H, HWP, masked, [0, 1] if masked else [], enc_of(cells))
        assert status == "err" and err == [1, 0, b, x, y, *bad]


def test_the_first_bad_cell_in_walk_order_is_the_one_named(codec_exe):
    cells = [{(1, 3): (T_KEY, 6, 0), (2, 0): (11, 0, 0)}, {(0, 0): (11, 0, 0)}]  # x-major: (1, 3) comes before (2, 0)
    status, err = run(codec_exe, "encode", B, W, H, HWP, 0, enc_of(cells))
    assert status == "err" and err == [1, 0, 0, 1, 3, T_KEY, 6, 0]


def test_contents_sit_on_box_cells_and_round_trip(codec_exe):
    grid = [{}, {(1, 3): (T_BOX, 2, 0), (2, 0): (T_BOX, 0, 0)}]
    _, cells = run(codec_exe, "encode", B, W, H, HWP, 0, enc_of(grid))
    held = [{(0, 1): (T_EMPTY, 4, 1), (2, 2): (0, 0, 0)},  # type <= 1 is nothing, on any cell
            {(1, 3): (T_KEY, 2, 0), (2, 0): (T_DOOR, 1, 2)}]
    status, plane = run(codec_exe, "contents", B, W, H, HWP, cells, enc_of(held))
    want = [0] * (B * HWP)
    want[plane_index(1, 1, 3)], want[plane_index(1, 2, 0)] = code(T_KEY, 2, 0), code(T_DOOR, 1, 2)
    assert status == "ok" and plane == want
    back = [0] * (B * W * H * 3)  # nothing held reads back as (0, 0, 0)
    for (x, y), tcs in held[1].items():
        i = ((1 * W + x) * H + y) * 3
        back[i:i + 3] = tcs
    assert run(codec_exe, "uncontents", B, W, H, HWP, plane) == back


def test_contents_refusals(codec_exe):
    grid = [{(2, 1): (T_BOX, 3, 0)}, {(0, 2): (T_BALL, 1, 0)}]
    _, cells = run(codec_exe, "encode", B, W, H, HWP, 0, enc_of(grid))

    def contents(b, x, y, tcs):
        held = [{}, {}]  # every other cell holds (T_EMPTY, 0, 0): nothing
        held[b][(x, y)] = tcs
        return run(codec_exe, "contents", B, W, H, HWP, cells, enc_of(held))

    assert contents(1, 0, 2, (T_KEY, 0, 0)) == ("err", [3, 0, 1, 0, 2, T_KEY, 0, 0])    # on a ball
    assert contents(0, 1, 1, (T_KEY, 0, 0)) == ("err", [3, 0, 0, 1, 1, T_KEY, 0, 0])    # on an empty cell
    assert contents(0, 2, 1, (T_AGENT, 0, 0)) == ("err", [2, 0, 0, 2, 1, T_AGENT, 0, 0])  # the agent is no object
    assert contents(0, 2, 1, (T_KEY, 6, 0)) == ("err", [2, 0, 0, 2, 1, T_KEY, 6, 0])
    assert contents(0, 2, 1, (T_KEY, 0, 1)) == ("err", [2, 0, 0, 2, 1, T_KEY, 0, 1])
    assert contents(0, 2, 1, (T_DOOR, 0, 3)) == ("err", [2, 0, 0, 2, 1, T_DOOR, 0, 3])
    assert contents(0, 2, 1, (16, 0, 0)) == ("err", [2, 0, 0, 2, 1, 16, 0, 0])           # would read back as a door
    assert contents(1, 0, 2, (T_EMPTY, 5, 2))[0] == "ok"


def test_carried_contents(codec_exe):
    status, codes = run(codec_exe, "carried", B, [T_BOX, 1, T_KEY, 0], [T_BALL, 1, 0, 0, 0, 0])
    assert status == "ok" and codes == [code(T_BALL, 1, 0), 0]
    assert run(codec_exe, "uncarried", B, codes) == [T_BALL, 1, 0, 0, 0, 0]
    assert run(codec_exe, "carried", B, [T_BOX, 1, T_KEY, 0], [0, 0, 0, T_BALL, 1, 0]) == ("err", [3, 1, 1, 0, 0, T_BALL, 1, 0])
    assert run(codec_exe, "carried", B, [T_BOX, 1, 0, 0], [T_AGENT, 0, 0, 0, 0, 0]) == ("err", [2, 1, 0, 0, 0, T_AGENT, 0, 0])
    assert run(codec_exe, "carried", B, [T_BOX, 1, 0, 0], [T_EMPTY, -1, 0, 0, 0, 0]) == ("err", [2, 1, 0, 0, 0, T_EMPTY, -1, 0])
    assert run(codec_exe, "carried", B, [0, 0, T_BOX, 0], [0, 0, 0, 1000, 0, 0]) == ("err", [2, 1, 1, 0, 0, 1000, 0, 0])


def test_agent_check(codec_exe):
    for x, y, d, ok in ((0, 0, 0, 1), (W - 1, H - 1, 3, 1), (W, 0, 0, 0), (0, H, 0, 0), (H - 1, 0, 0, 0), (-1, 0, 0, 0),
                        (0, -1, 0, 0), (0, 0, 4, 0), (0, 0, -1, 0)):
        assert run(codec_exe, "agent", W, H, x, y, d) == [ok], (x, y, d)


@pytest.mark.parametrize("nb", [2, 17])  # 2 * 17 crosses a 16-byte boundary
def test_staging_layout(codec_exe, nb):
    mask, see, cells, agent, carry, mx, total = run(codec_exe, "stage", nb, HWP)
    assert cells % 16 == 0 and HWP % 16 == 0  # the kernel reads each env's cells as uint4
    assert agent % 4 == 0 and carry % 4 == 0 and mx % 4 == 0
    sections = [(mask, nb), (see, nb), (cells, nb * HWP), (agent, 16 * nb), (carry, 8 * nb), (mx, 4 * nb)]
    for (o0, n0), (o1, _) in zip(sections, sections[1:]):
        assert o0 + n0 <= o1
    assert mask == 0 and mx + 4 * nb == total
    assert total == (2 * nb + 15) // 16 * 16 + nb * HWP + 4 * 7 * nb  # mgdp_envs_load's size before the layout was a struct
