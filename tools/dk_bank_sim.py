"""LDS bank-conflict model of the batched DoorKey-16 tile accesses (MI355X_MICROARCH.md §LDS:
ds_read_b128 = 4 groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... on (a/4) mod 64;
ds_write_b128 = 8 groups of 8 contiguous lanes on (a/4) mod 32; each extra distinct address on a
busy 16-B slot of a group costs one LDS cycle).  Per grid-sweep LDS-array cycles of:
  cellperm  fused_fast_dk_soa with the special-first thread -> cell map (round 4's default),
  identity  fused_fast_dk_soa with thread t on cell t (tried and measured slower: profiles/r03_dk/perm/),
  rows      fused_dk_rows (whole rows per 16 lanes, planes 1 / 3 only, DPP east / west).
Grids: tests/golden/grids_doorkey16.npz (reference-generated).  Run: python tools/dk_bank_sim.py"""
import os

import numpy as np

E, WALL, FLOOR, DOOR, KEY, GOAL, LAVA = 1, 2, 3, 4, 5, 8, 9


def walkmask(t):
    m = 0
    for hk in range(2):
        for dop in range(2):
            if t in (E, FLOOR) or (t == DOOR and dop) or (t == KEY and hk):
                m |= 1 << (hk * 2 + dop)
    return m


G_R128 = [[0, 1, 2, 3, 12, 13, 14, 15] + list(range(20, 28)), list(range(4, 12)) + [16, 17, 18, 19] + list(range(28, 32))]
G_R128 += [[l + 32 for l in g] for g in G_R128]
G_W128 = [list(range(i * 8, i * 8 + 8)) for i in range(8)]


def cycles(addrs, groups, slots):
    tot = 0
    for g in groups:
        per = {}
        for l in g:
            per.setdefault((addrs[l] // 16) % slots, set()).add(addrs[l])
        tot += max([len(s) for s in per.values()] + [1])
    return tot


def cell_info(types, W):
    HW = len(types)
    off = [1, W, -1, -W]
    info = []
    for c in range(HW):
        t = types[c]
        walk = walkmask(t)
        f, nb = [], []
        for d in range(4):
            cfr = c + off[d] if walk else c
            tf = types[cfr] if walk else WALL
            fm = walkmask(tf) | (16 if tf == GOAL else 0) | (32 if tf == LAVA else 0) | (64 if tf == KEY else 0) | (128 if tf == DOOR else 0)
            reads = walk != 0 and not (fm & 48) and (fm & 15) != 0
            nb.append(cfr if reads else None)  # None: cell 0's group (dk_fast_topo)
            f.append(fm if walk else 0)
        goal = any(x & 16 for x in f)
        kd = (walk not in (0, 15)) or any(x & 192 for x in f)
        info.append((walk, nb, goal, kd))
    return info


def soa(types, W, perm_on):
    HW = len(types)
    HWs = (HW + 63) // 64 * 64
    info = cell_info(types, W)
    if perm_on:
        sp = [c for c in range(HW) if info[c][2] or info[c][3]]
        pl = [c for c in range(HW) if not (info[c][2] or info[c][3]) and info[c][0]]
        ab = [c for c in range(HW) if not (info[c][2] or info[c][3]) and not info[c][0]]
        perm = sp + pl + ab
    else:
        perm = list(range(HW))
    cyc = mn = 0
    for w in range(HWs // 64):
        cells = [perm[t] if t < HW else t for t in range(w * 64, w * 64 + 64)]
        dead = perm_on and all(info[c][0] == 0 for c in cells if c < HW)
        for d in range(4):
            base = d * HWs * 16
            cyc += cycles([base + c * 16 for c in cells], G_W128, 8)
            mn += 8
            if not dead:
                ra = [base + ((info[c][1][d] if c < HW else None) or 0) * 16 for c in cells]
                cyc += cycles(ra, G_R128, 16)
                mn += 4
    return cyc, mn


def rows(types, W):
    assert W == 16
    HW = len(types)
    HWs = (HW + 63) // 64 * 64
    info = cell_info(types, W)
    nrow = HWs // 16
    key = []
    for r in range(nrow):
        cs = range(r * 16, min(r * 16 + 16, HW))
        k = 0
        if r * 16 < HW:
            k = (8 if any(info[c][3] for c in cs) else 0) | (4 if any(info[c][2] for c in cs) else 0) | \
                (2 if any(info[c][0] for c in cs) else 0) | 1
        key.append(k)
    order = sorted(range(nrow), key=lambda r: (-key[r], r))
    PL = HWs + 32
    cyc = mn = 0
    for w in range(HWs // 64):
        cells = [order[(w * 64 + l) >> 4] * 16 + (l & 15) for l in range(64)]
        for p, delta in ((0, 16), (1, -16)):  # plane 1 read at c + 16, plane 3 at c - 16
            base = p * PL * 16
            cyc += cycles([base + (16 + c) * 16 for c in cells], G_W128, 8)
            cyc += cycles([base + (16 + c + delta) * 16 for c in cells], G_R128, 16)
            mn += 12
    return cyc, mn


def main():
    d = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "grids_doorkey16.npz"))
    for name, fn in (("cellperm", lambda t: soa(t, 16, True)), ("identity", lambda t: soa(t, 16, False)),
                     ("rows", lambda t: rows(t, 16))):
        cyc = mn = 0
        for g in range(d["enc"].shape[0]):
            c, m = fn(d["enc"][g, :, :, 0].T.flatten().astype(int))
            cyc += c
            mn += m
        n = d["enc"].shape[0]
        print(f"{name:9s} LDS-array cycles per grid-sweep {cyc / n:7.1f} (conflict-free {mn / n:6.1f}), "
              f"conflict share {(cyc - mn) / cyc:.3f}")


if __name__ == "__main__":
    main()


def wave_classes(types, W, mode):
    """Per wave of one grid: 'kd', 'goal', 'plain' or 'dead' (cellperm only) for the thread -> cell
    map of `mode` (VALU form each wave of the sweep takes)."""
    HW = len(types)
    HWs = (HW + 63) // 64 * 64
    info = cell_info(types, W)
    if mode == "rows":
        nrow = HWs // 16
        key = []
        for r in range(nrow):
            cs = range(r * 16, min(r * 16 + 16, HW))
            key.append(((8 if any(info[c][3] for c in cs) else 0) | (4 if any(info[c][2] for c in cs) else 0) |
                        (2 if any(info[c][0] for c in cs) else 0) | 1) if r * 16 < HW else 0)
        order = sorted(range(nrow), key=lambda r: (-key[r], r))
        perm = [order[t >> 4] * 16 + (t & 15) for t in range(HWs)]
    elif mode == "cellperm":
        sp = [c for c in range(HW) if info[c][2] or info[c][3]]
        pl = [c for c in range(HW) if not (info[c][2] or info[c][3]) and info[c][0]]
        ab = [c for c in range(HW) if not (info[c][2] or info[c][3]) and not info[c][0]]
        perm = sp + pl + ab + list(range(HW, HWs))
    else:
        perm = list(range(HWs))
    out = []
    for w in range(HWs // 64):
        cells = [c for c in perm[w * 64:(w + 1) * 64] if c < HW]
        if mode == "cellperm" and all(info[c][0] == 0 for c in cells):
            out.append("dead")
        elif any(info[c][3] for c in cells):
            out.append("kd")
        elif any(info[c][2] for c in cells):
            out.append("goal")
        else:
            out.append("plain")
    return out


def classes_main():
    import collections

    d = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "grids_doorkey16.npz"))
    for mode in ("identity", "cellperm", "rows"):
        cnt = collections.Counter()
        for g in range(d["enc"].shape[0]):
            cnt.update(wave_classes(d["enc"][g, :, :, 0].T.flatten().astype(int), 16, mode))
        n = d["enc"].shape[0]
        print(f"{mode:9s} waves per grid by form: " + ", ".join(f"{k} {v / n:.2f}" for k, v in sorted(cnt.items())))
