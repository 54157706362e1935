"""Finite-horizon policy evaluation against the horizon solve on one handle:
kernel microseconds, from the handle's HIP events, of

    a  solve() with keep_policy_t       the options kernel doing the same H sweeps (the yardstick)
    b  evaluate_opts_device(None, T=H)  the handle's own pi_t: one row of lanes read per sweep
    c  b with V_t                       plus one row of values written per sweep
    d  evaluate_opts_device(None, T=1)  a stationary pi: lanes in registers, nothing per sweep

The sides alternate within a repetition; the figure is the median of --reps repetitions with min-max
(and the median wall time of the whole call).
b (and c) must reproduce the solve's V_0 bit for bit (checked).  Also prints the bytes of the pi_t read
and of the V_t write and their time at the streaming-copy rate, so the bound that applies can be named.
The prefetch distance is a compile-time constant (MGDP_EVAL_PF): build one library per distance
(MGDP_BUILD_OUT=... MGDP_EXTRA_FLAGS=-DMGDP_EVAL_PF=n) and run this probe once per library with
MGDP_LIB set and --tag naming it.  One JSON line per workload; --out appends them to a file.

    python tools/probe_eval_opts.py [--out profiles/eval_opts/probe_eval_opts.jsonl] [--reps 5] [--tag pf4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (env, B, handle options); H is the env's own max_steps
WORKLOADS = [("MiniGrid-LavaCrossingS11N5-v0", 4096, {}),
             ("MiniGrid-LavaCrossingS11N5-v0", 4096, {"lava": "nodeath", "death_cost": -0.05}),
             ("MiniGrid-DoorKey-8x8-v0", 4096, {})]
HBM_BPS = 6.0e12  # streaming-copy rate measured on this pool (6.0-6.3 TB/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sides", default="abcd")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    ap.add_argument("--only", type=int, default=-1, help="run one workload by index")
    args = ap.parse_args()
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    for i, (env, B, opts) in enumerate(WORKLOADS):
        if args.only >= 0 and i != args.only:
            continue
        B = max(1, int(B * args.scale))
        H = mg.make(env).max_steps
        cells = gen.generate(env, 0, B, enc=False, cells=True, agent=False)["cells"]
        vi = mg.ValueIteration(cells, dtype="f32", gamma=1.0, horizon=H, keep_policy_t=True, **opts)
        assert vi.solve() == H
        V = vi.values()
        d_vt = torch.empty((H, B, vi.S), dtype=torch.float32, device="cuda") if "c" in args.sides else None
        calls = {"a": vi.solve, "b": lambda: vi.evaluate_opts_device(None, T=H),
                 "c": lambda: vi.evaluate_opts_device(None, T=H, values_t_ptr=d_vt.data_ptr()),
                 "d": lambda: vi.evaluate_opts_device(None, T=1)}
        for s in args.sides:  # warm-up, and the checks
            assert calls[s]() == H
            if s in "abc":
                assert np.array_equal(vi.values(), V), f"side {s}: V_0 differs from the solve's"
        if d_vt is not None:
            assert np.array_equal(d_vt[0].cpu().numpy(), V)
        vi.enable_timing(True)
        us = {s: [] for s in args.sides}
        wall = {s: [] for s in args.sides}
        launches = {}
        for _ in range(args.reps):
            for s in args.sides:  # alternating: every side sees the same clocks and neighbours
                ms0, n0 = vi.kernel_time()
                t = time.perf_counter()
                calls[s]()
                wall[s].append((time.perf_counter() - t) * 1e6)
                ms1, n1 = vi.kernel_time()
                us[s].append((ms1 - ms0) * 1e3)
                launches[s] = n1 - n0
        pi_bytes, vt_bytes = H * B * vi.S, H * B * vi.S * 4
        rec = {"env": env, "B": B, "H": H, "opts": opts, "box": box, "tag": args.tag, "lib": os.path.basename(_lib.lib_path()),
               "pi_t_bytes": pi_bytes, "pi_t_hbm_floor_us": round(pi_bytes / HBM_BPS * 1e6, 1),
               "v_t_bytes": vt_bytes, "v_t_hbm_floor_us": round(vt_bytes / HBM_BPS * 1e6, 1)}
        for s in args.sides:
            rec[f"{s}_us"] = round(float(np.median(us[s])), 1)
            rec[f"{s}_us_min_max"] = [round(min(us[s]), 1), round(max(us[s]), 1)]
            rec[f"{s}_us_per_sweep"] = round(float(np.median(us[s])) / H, 4)
            rec[f"{s}_launches"] = launches[s]
            rec[f"{s}_wall_us"] = round(float(np.median(wall[s])), 1)  # the whole call, host side included
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        vi.close()
        del d_vt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
