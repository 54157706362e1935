"""The fused policy rollout against the two ways the same job was done before it, in one session:
  (a) envs_rollout_kernel: pi* of a solved handle (zero copy) rolled out to completion in one launch --
      kernel time from the handle's HIP-event timing; also with the HBM cell reader forced
      (MGDP_ROLLOUT_READER=hbm), the A/B of DESIGN.md section 16;
  (b) the same number of envs_step_kernel launches (mgdp_envs_step_device) on the same envs with the
      rollout's own actions precomputed on the device -- the per-step path, kernel time only;
  (c) the host loop of tests/test_gpu_rollout.py (get_state, a Python state index and table lookup per
      env, one step() per env step) -- wall time, on the first --host-envs envs of the batch.
(a) and (b) alternate inside every repetition; medians over the repetitions with min-max.  One JSON
line per workload; --out appends them to a file.

    python tools/probe_rollout.py [--out profiles/rollout/probe_rollout.jsonl] [--reps 5] [--host-envs 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [("MiniGrid-DoorKey-16x16-v0", 65536, "doorkey"), ("MiniGrid-FourRooms-v0", 4096, "xyd")]


def stats(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2)}


def host_loop(mg, env_id, enc, agent, res, model):
    """tests/test_gpu_rollout.py's loop: the only way to roll a policy out before the fused kernel."""
    from minigrid_dynamicprogramming_amd.core import OBJECT_TO_IDX

    B = enc.shape[0]
    venv = mg.MiniGridVecEnv(env_id, B)
    venv.load(enc, agent)
    door = None
    if model == "doorkey":
        door = [tuple(np.argwhere(enc[b, :, :, 0] == OBJECT_TO_IDX["door"])[0]) for b in range(B)]

    def states(st):
        out = []
        for b in range(B):
            x, y, d = (int(v) for v in st["agent"][b])
            hk = dop = 0
            if model == "doorkey":
                hk = int(st["carry"][b, 0] == OBJECT_TO_IDX["key"])
                dop = int(st["enc"][b, door[b][0], door[b][1], 2] == 0)
            out.append((x, y, d, hk, dop))
        return out

    t0 = time.perf_counter()
    st = venv.get_state()
    done = np.zeros(B, bool)
    steps = np.zeros(B, np.int64)
    n = 0
    while not done.all():
        cur = states(st)
        acts = np.array([res.action(b, *cur[b]) if not done[b] else 6 for b in range(B)])
        acts[acts < 0] = 6
        _, _, term, trunc, _ = venv.step(acts)
        steps[~done] += 1
        done |= term | trunc
        st = venv.get_state()
        n += 1
    wall = time.perf_counter() - t0
    venv.close()
    return wall, n, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-envs", type=int, default=4096)
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    args = ap.parse_args()
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    dev = torch.device("cuda", 0)
    for env_id, B, model in WORKLOADS:
        B = max(1, int(B * args.scale))
        g = gen.generate(env_id, 0, B)
        enc, agent = g["enc"], g["agent"]
        vi = mg.ValueIteration(enc, model=model, dtype="f32")
        vi.solve()
        pi_ptr = vi.device_buffers()[1]
        res = vi.result()

        def make(**env):
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                return mg.MiniGridVecEnv(env_id, B)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

        venvs = {"lds": make(), "hbm_reader": make(MGDP_ROLLOUT_READER="hbm")}
        steps = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        ret = torch.zeros(B, dtype=torch.float64, device=dev)
        term = torch.zeros(B, dtype=torch.uint8, device=dev)
        trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
        V = venvs["lds"].view
        obs = torch.zeros((B, V, V, 3), dtype=torch.uint8, device=dev)
        direction = torch.zeros(B, dtype=torch.int32, device=dev)
        rew = torch.zeros(B, dtype=torch.float64, device=dev)
        sstat = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        # one traced rollout: the actions of every step, for (b), and the reference outputs of the A/B sides
        v0 = venvs["lds"]
        v0.load(enc, agent)
        v0.rollout_device(pi_ptr, 1, model, None, steps, ret, term, trunc, status)
        v0.kernel_time()
        torch.cuda.synchronize()
        ref_steps, ref_ret = steps.cpu().numpy().copy(), ret.cpu().numpy().copy()
        assert (status.cpu().numpy() == 0).all()
        n_launch = int(ref_steps.max())  # the longest episode: the trace's length and (b)'s launches
        tr_s = torch.zeros((n_launch, B), dtype=torch.int32, device=dev)
        tr_a = torch.zeros((n_launch, B), dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        v0.load(enc, agent)
        v0.rollout_device(pi_ptr, 1, model, None, steps, ret, term, trunc, status, tr_s, tr_a, n_launch)
        v0.kernel_time()
        torch.cuda.synchronize()
        assert np.array_equal(steps.cpu().numpy(), ref_steps)
        acts = tr_a.to(torch.int32)
        acts[acts < 0] = 6  # an env that has ended: "done"
        acts = acts.contiguous()
        torch.cuda.synchronize()
        raw = [t.data_ptr() for t in (obs, direction, rew, term, trunc, sstat)]
        for v in venvs.values():
            v.enable_timing(True)
        times = {k: [] for k in list(venvs) + ["step_device"]}
        for _ in range(args.reps):
            for name, v in venvs.items():  # (a), each side of the A/Bs ...
                v.load(enc, agent)
                ms0, n0 = v.kernel_time()
                v.rollout_device(pi_ptr, 1, model, None, steps, ret, term, trunc, status)
                ms1, n1 = v.kernel_time()
                assert n1 - n0 == 1
                times[name].append((ms1 - ms0) * 1e3)
                torch.cuda.synchronize()
                assert np.array_equal(steps.cpu().numpy(), ref_steps) and np.array_equal(ret.cpu().numpy(), ref_ret), name
            v0.load(enc, agent)  # ... then (b) on the same envs
            ms0, n0 = v0.kernel_time()
            for t in range(n_launch):
                v0.step_device(acts[t].data_ptr(), *raw)
            ms1, n1 = v0.kernel_time()
            assert n1 - n0 == n_launch
            times["step_device"].append((ms1 - ms0) * 1e3)
        for v in venvs.values():
            v.close()
        Bc = min(B, args.host_envs)
        sub = mg.VIResult(res.V[:Bc], res.pi[:Bc], res.sweeps, res.converged, res.dv, res.model, res.W, res.H)
        wall, n_host, host_steps = host_loop(mg, env_id, enc[:Bc], agent[:Bc], sub, model)
        assert np.array_equal(host_steps, ref_steps[:Bc]), "the host loop and the rollout took different steps"
        vi.close()
        total = int(ref_steps.sum())
        a, b = stats(times["lds"]), stats(times["step_device"])
        rec = {"env": env_id, "B": B, "model": model, "box": box, "reps": args.reps,
               "env_steps": total, "max_steps_per_env": n_launch, "mean_steps_per_env": round(total / B, 2),
               "reached_goal": int((ref_ret > 0).sum()),
               "a_rollout_kernel_us": a, "b_step_device_kernel_us": b, "b_launches": n_launch,
               "a_over_b": round(a["median"] / b["median"], 4),
               "a_env_steps_per_s": round(total / (a["median"] * 1e-6), 1),
               "a_hbm_reader_kernel_us": stats(times["hbm_reader"]),
               "c_host_loop_envs": Bc, "c_host_loop_wall_s": round(wall, 3), "c_host_loop_steps": n_host,
               "c_wall_us_per_env_step": round(wall * 1e6 / max(int(host_steps.sum()), 1), 3),
               "a_kernel_us_per_env_step": round(a["median"] / total, 6)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
