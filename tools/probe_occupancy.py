"""The forward pass of a policy beside its backward evaluation on one handle:
kernel microseconds, from the handle's HIP events, of

    e1  evaluate_opts_device(pi_0, T=1)        o1  occupancy_device(pi_0, T=1)       stationary lanes in registers
    e2  evaluate_opts_device(pi_t, T=H)        o2  occupancy_device(pi_t, T=H)       one row of lanes read per sweep
    e3  e2 with V_t                            o3  o2 with mu_t                      plus one row of values written

on the same policy (the horizon solve's own pi_t, copied to device memory once) and, for the forward sides,
from each env's start state.  The sides alternate within a repetition after a warm-up call of each; the
figure is the median of --reps repetitions with min-max.  The forward pass is checked on the way: without
slip and with gamma = 1 its expected_return from the start state is the solve's V_0[start] bit for bit.
One JSON line per workload; --out appends them to a file.

    python tools/probe_occupancy.py [--out profiles/occupancy/probe_occupancy.jsonl] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (env, B, handle options); H is the env's own max_steps (484 and 100)
WORKLOADS = [("MiniGrid-LavaCrossingS11N5-v0", 4096, {}),
             ("MiniGrid-FourRooms-v0", 4096, {}),
             ("MiniGrid-LavaCrossingS11N5-v0", 4096, {"slip_p": 0.9}),
             ("MiniGrid-FourRooms-v0", 4096, {"slip_p": 0.9})]
SIDES = ("e1", "o1", "e2", "o2", "e3", "o3")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    ap.add_argument("--only", type=int, default=-1, help="run one workload by index")
    args = ap.parse_args()
    sides = [s for s in args.sides.split(",") if s]
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen
    from minigrid_dynamicprogramming_amd.dp import state_index

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    tdt = torch.float32 if args.dtype == "f32" else torch.float64
    for i, (env, B, opts) in enumerate(WORKLOADS):
        if args.only >= 0 and i != args.only:
            continue
        B = max(1, int(B * args.scale))
        H = mg.make(env).max_steps
        g = gen.generate(env, 0, B, enc=False, cells=True, agent=True)
        cells, agent = g["cells"], g["agent"]
        vi = mg.ValueIteration(cells, dtype=args.dtype, gamma=1.0, horizon=H, keep_policy_t=True, **opts)
        assert vi.solve() == H
        V = vi.values()
        start = np.array([state_index("xyd", vi.W, *(int(v) for v in agent[b])) for b in range(B)], np.int32)
        d_pi = torch.from_numpy(vi.policy_t()).cuda()
        d_start = torch.from_numpy(start).cuda()
        mu, occ, ret = (torch.empty((B, vi.S), dtype=tdt, device="cuda") for _ in range(3))
        big = torch.empty((H, B, vi.S), dtype=tdt, device="cuda") if ("e3" in sides or "o3" in sides) else None
        torch.cuda.synchronize()
        fwd = dict(start_ptr=d_start.data_ptr(), occ_ptr=occ.data_ptr(), ret_ptr=ret.data_ptr())
        calls = {"e1": lambda: vi.evaluate_opts_device(d_pi.data_ptr(), T=1),
                 "e2": lambda: vi.evaluate_opts_device(d_pi.data_ptr(), T=H),
                 "e3": lambda: vi.evaluate_opts_device(d_pi.data_ptr(), T=H, values_t_ptr=big.data_ptr()),
                 "o1": lambda: vi.occupancy_device(d_pi.data_ptr(), 1, mu.data_ptr(), **fwd),
                 "o2": lambda: vi.occupancy_device(d_pi.data_ptr(), H, mu.data_ptr(), **fwd),
                 "o3": lambda: vi.occupancy_device(d_pi.data_ptr(), H, mu.data_ptr(), mu_t_ptr=big.data_ptr(), **fwd)}
        gap = None
        for s in sides:  # warm-up, and the checks
            assert calls[s]() == H
            if s in ("e2", "e3"):
                assert np.array_equal(vi.values(), V), f"side {s}: V_0 differs from the solve's"
            if s in ("o2", "o3"):
                er = ret.cpu().numpy().sum(axis=1, dtype=np.float64)
                v0 = V[np.arange(B), start].astype(np.float64)
                if "slip_p" not in opts:
                    assert np.array_equal(er.astype(V.dtype), V[np.arange(B), start]), f"side {s}: sum ret differs from V_0[start]"
                gap = float(np.abs(er - v0).max())
        vi.enable_timing(True)
        us = {s: [] for s in sides}
        for _ in range(args.reps):
            for s in sides:  # alternating: every side sees the same clocks and neighbours
                ms0, _ = vi.kernel_time()
                calls[s]()
                ms1, _ = vi.kernel_time()
                us[s].append((ms1 - ms0) * 1e3)
        rec = {"env": env, "B": B, "H": H, "dtype": args.dtype, "opts": opts, "box": box,
               "lib": os.path.basename(_lib.lib_path()), "reps": args.reps, "max_gap_sum_ret_vs_v0": gap}
        for s in sides:
            rec[f"{s}_us"] = round(float(np.median(us[s])), 1)
            rec[f"{s}_us_min_max"] = [round(min(us[s]), 1), round(max(us[s]), 1)]
            rec[f"{s}_us_per_step"] = round(float(np.median(us[s])) / H, 4)
        for k in "123":
            if f"e{k}" in sides and f"o{k}" in sides:
                rec[f"o{k}_over_e{k}"] = round(rec[f"o{k}_us"] / rec[f"e{k}_us"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        vi.close()
        del big, d_pi, mu, occ, ret
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
