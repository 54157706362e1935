"""The slip rollout against the per-step path and against the plain rollout, in one
session.  pi* comes from a solved slip_p handle, read in place; the envs run to completion under
set_slip(slip_p, seed).
  (a) envs_rollout_kernel<.., SLIP = true>: one launch, kernel time from the handle's HIP-event timing;
  (b) the same episode lengths as per-step launches of policy_actions_device + slip_actions_device +
      step_device on the same envs from the same seed, kernel time summed over all three kernels;
  (c) the plain rollout (no slip) of the same policy on the same envs: kernel time per env-step against
      (a)'s -- what the stream costs per step.
The three sides alternate inside every repetition; medians over the repetitions with min-max.  (b) must
leave the streams (a) left, and every repetition of (a) the steps and returns of the first (asserted).
Last, untimed: the same rollout with max_steps loaded as --mc-max-steps (no episode is cut short), and the
Monte-Carlo mean of g = gamma^(steps-1) on the goal, 0 elsewhere, against V*[start] of each env's own grid
(z of the paired differences).  One JSON line per workload; --out appends them to a file.

    python tools/probe_slip_rollout.py [--out profiles/slip_rollout/probe_slip_rollout.jsonl] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [("MiniGrid-FourRooms-v0", 4096), ("MiniGrid-LavaCrossingS11N5-v0", 65536)]


def stats(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slip-p", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mc-max-steps", type=int, default=4096)
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    args = ap.parse_args()
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen
    from minigrid_dynamicprogramming_amd.dp import state_index

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    dev = torch.device("cuda", 0)
    p, model = args.slip_p, "xyd"
    for env_id, B in WORKLOADS:
        B = max(1, int(B * args.scale))
        g = gen.generate(env_id, 0, B)
        enc, agent = g["enc"], g["agent"]
        vi = mg.ValueIteration(enc, model=model, dtype="f64", tol=1e-10, slip_p=p)
        vi.solve()
        pi_ptr = vi.device_buffers()[1]
        gamma = 0.99  # ValueIteration's default
        V = vi.values()
        start = np.array([state_index(model, vi.W, int(a[0]), int(a[1]), int(a[2]), 0, 0) for a in agent])
        v_start = V[np.arange(B), start].astype(np.float64)

        slip = mg.MiniGridVecEnv(env_id, B)   # (a) and (c) share nothing but the policy
        loop = mg.MiniGridVecEnv(env_id, B)   # (b)
        plain = mg.MiniGridVecEnv(env_id, B)  # (c)
        steps = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        ret = torch.zeros(B, dtype=torch.float64, device=dev)
        term = torch.zeros(B, dtype=torch.uint8, device=dev)
        trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
        act = torch.zeros(B, dtype=torch.int32, device=dev)
        lstat = torch.zeros(B, dtype=torch.int32, device=dev)
        Vw = slip.view
        obs = torch.zeros((B, Vw, Vw, 3), dtype=torch.uint8, device=dev)
        direction = torch.zeros(B, dtype=torch.int32, device=dev)
        rew = torch.zeros(B, dtype=torch.float64, device=dev)
        sstat = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        raw = [t.data_ptr() for t in (obs, direction, rew, term, trunc, sstat)]

        def fused(v, with_slip):
            v.load(enc, agent)
            if with_slip:
                v.set_slip(p, seed=args.seed)
            ms0, n0 = v.kernel_time()
            v.rollout_device(pi_ptr, 1, model, None, steps, ret, term, trunc, status)
            ms1, n1 = v.kernel_time()
            assert n1 - n0 == 1
            torch.cuda.synchronize()
            return (ms1 - ms0) * 1e3, steps.cpu().numpy().copy(), ret.cpu().numpy().copy()

        for v in (slip, loop, plain):
            v.enable_timing(True)
        _, ref_steps, ref_ret = fused(slip, True)  # also the warm-up of (a)
        assert (status.cpu().numpy() == 0).all()
        # an env cut off by max_steps stops in (a) and is stepped on by (b)'s loop: its stream is not compared
        ran_out = trunc.cpu().numpy().astype(bool)
        ref_streams = slip.slip_streams()
        n_launch = int(ref_steps.max())
        _, plain_steps, plain_ret = fused(plain, False)
        times = {"a": [], "b": [], "c": []}
        for _ in range(args.reps):
            t, s, r = fused(slip, True)
            assert np.array_equal(s, ref_steps) and np.array_equal(r, ref_ret)
            times["a"].append(t)
            loop.load(enc, agent)
            loop.set_slip(p, seed=args.seed)
            ms0, n0 = loop.kernel_time()
            for _k in range(n_launch):  # an ended env: -1 from the lookup, passed through, refused by step
                loop.policy_actions_device(pi_ptr, 1, model, act, lstat)
                loop.slip_actions_device(act, act)
                loop.step_device(act.data_ptr(), *raw)
            ms1, n1 = loop.kernel_time()
            assert n1 - n0 == 3 * n_launch
            times["b"].append((ms1 - ms0) * 1e3)
            got = loop.slip_streams()
            assert all(np.array_equal(got[k][~ran_out], ref_streams[k][~ran_out]) for k in got), "(b) drew differently from (a)"
            t, s, r = fused(plain, False)
            assert np.array_equal(s, plain_steps) and np.array_equal(r, plain_ret)
            times["c"].append(t)
        # Monte Carlo against the DP, untimed: no truncation
        slip.load(enc, agent, max_steps=args.mc_max_steps)
        slip.set_slip(p, seed=args.seed)
        slip.rollout_device(pi_ptr, 1, model, None, steps, ret, term, trunc, status)
        slip.kernel_time()
        torch.cuda.synchronize()
        mc_steps, mc_ret = steps.cpu().numpy(), ret.cpu().numpy()
        hit = term.cpu().numpy().astype(bool) & (mc_ret > 0)
        gq = np.where(hit, gamma ** (mc_steps.astype(np.float64) - 1.0), 0.0)
        diff = gq - v_start
        z = float(diff.mean() / (diff.std(ddof=1) / np.sqrt(B))) if B > 1 else 0.0
        for v in (slip, loop, plain):
            v.close()
        vi.close()
        total, total_plain = int(ref_steps.sum()), int(plain_steps.sum())
        a, b, c = stats(times["a"]), stats(times["b"]), stats(times["c"])
        a_step, c_step = a["median"] / total, c["median"] / total_plain
        rec = {"env": env_id, "B": B, "model": model, "box": box, "reps": args.reps, "slip_p": p, "seed": args.seed,
               "env_steps": total, "max_steps_per_env": n_launch, "mean_steps_per_env": round(total / B, 2),
               "reached_goal": int((ref_ret > 0).sum()), "truncated": int(ran_out.sum()),
               "a_slip_rollout_kernel_us": a, "b_per_step_kernel_us": b, "b_launches": 3 * n_launch,
               "a_over_b": round(a["median"] / b["median"], 4),
               "c_plain_rollout_kernel_us": c, "c_env_steps": total_plain,
               "a_kernel_ns_per_env_step": round(a_step * 1e3, 4), "c_kernel_ns_per_env_step": round(c_step * 1e3, 4),
               "a_over_c_per_env_step": round(a_step / c_step, 3),
               "a_env_steps_per_s": round(total / (a["median"] * 1e-6), 1),
               "mc_max_steps": args.mc_max_steps, "mc_truncated": int(trunc.cpu().numpy().sum()),
               "mc_mean_g": round(float(gq.mean()), 6), "mc_mean_v_start": round(float(v_start.mean()), 6),
               "mc_z": round(z, 3), "gamma": gamma}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
