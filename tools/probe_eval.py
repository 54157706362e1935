"""Policy evaluation against the solve on one handle: alternate solve() and evaluate(pi*) with launch
timing on and report kernel microseconds per call of each, and their ratio.  pi* of deterministic
grids makes the evaluation run exactly the solve's K sweeps (checked, with V), so the two times are
directly comparable: the solve goes through the handle's planned loop, the evaluation through
vi_eval_kernel's barrier-per-sweep workgroup.  Also prints the evaluation's two bandwidth floors
(HBM: cells + pi in, pi + V out, once; LDS: own + front reads and the own writes of every executed
sweep) so the bound that applies can be named.  One JSON line per workload; --out appends them to a file.

    python tools/probe_eval.py [--out profiles/eval/probe_eval.json] [--reps 5] [--calls 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [("MiniGrid-Empty-16x16-v0", 65536), ("MiniGrid-FourRooms-v0", 4096)]
HBM_BPS = 6.3e12       # achievable HBM3E rate (8 TB/s spec)
LDS_READ_BPS = 75e12   # ds_read_b32, every CU streaming
LDS_WRITE_BPS = 45e12  # ds_write_b32 (38-51 TB/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    args = ap.parse_args()
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    for env, B in WORKLOADS:
        B = max(1, int(B * args.scale))
        cells = gen.generate(env, 0, B, enc=False, cells=True, agent=False)["cells"]
        vi = mg.ValueIteration(cells, dtype=args.dtype)
        k = vi.solve()
        V, pi = vi.values(), vi.policy()
        assert vi.evaluate_device() == k, "pi* of a deterministic batch evaluates in the solve's K sweeps"
        assert np.array_equal(vi.values(), V) and np.array_equal(vi.policy(), pi)
        executed = float(vi.grid_sweeps().mean())
        vi.enable_timing(True)  # launches from here on are timed; a timed batch solve is a launch
        solve_us, eval_us, solve_wall, eval_wall, launches = [], [], [], [], []
        for _ in range(args.reps):
            acc = {"s": 0.0, "e": 0.0, "sw": 0.0, "ew": 0.0, "sl": 0, "el": 0}
            ms0, n0 = vi.kernel_time()
            for _ in range(args.calls):  # alternating: both see the same clocks and neighbours
                t = time.perf_counter()
                vi.solve()
                acc["sw"] += time.perf_counter() - t
                ms1, n1 = vi.kernel_time()
                t = time.perf_counter()
                vi.evaluate_device()
                acc["ew"] += time.perf_counter() - t
                ms2, n2 = vi.kernel_time()
                acc["s"] += ms1 - ms0
                acc["e"] += ms2 - ms1
                acc["sl"] += n1 - n0
                acc["el"] += n2 - n1
                ms0, n0 = ms2, n2
            solve_us.append(acc["s"] * 1e3 / args.calls)
            eval_us.append(acc["e"] * 1e3 / args.calls)
            solve_wall.append(acc["sw"] * 1e6 / args.calls)
            eval_wall.append(acc["ew"] * 1e6 / args.calls)
            launches.append((acc["sl"] / args.calls, acc["el"] / args.calls))
        S, ts = vi.S, 4 if args.dtype == "f32" else 8
        hbm_bytes = B * (vi.W * vi.H + 2 * S + S * ts)
        lds_read = B * executed * 2 * S * ts
        lds_write = B * executed * S * ts
        s_med, e_med = float(np.median(solve_us)), float(np.median(eval_us))
        rec = {"env": env, "B": B, "dtype": args.dtype, "box": box, "sweeps": k, "mean_executed_sweeps": round(executed, 2),
               "solve_variant": vi.variant, "solve_kernel_us": round(s_med, 2), "eval_kernel_us": round(e_med, 2),
               "eval_over_solve": round(e_med / s_med, 3),
               "solve_wall_us": round(float(np.median(solve_wall)), 1), "eval_wall_us": round(float(np.median(eval_wall)), 1),
               "launches_per_solve": launches[-1][0], "launches_per_eval": launches[-1][1],
               "eval_hbm_bytes": hbm_bytes, "eval_hbm_floor_us": round(hbm_bytes / HBM_BPS * 1e6, 2),
               "eval_lds_floor_us": round((lds_read / LDS_READ_BPS + lds_write / LDS_WRITE_BPS) * 1e6, 2),
               "solve_kernel_us_all": [round(x, 2) for x in solve_us], "eval_kernel_us_all": [round(x, 2) for x in eval_us]}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        vi.close()


if __name__ == "__main__":
    main()
