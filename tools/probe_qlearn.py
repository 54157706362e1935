"""Tabular Q-learning on resident envs against the plain rollout, in one session.
Per workload the envs are loaded once with max_steps = n_steps (so a time-indexed policy of n_steps rows covers
every step_count) and both sides run on that one handle:
  (a) envs_qlearn_kernel: n_steps eps-greedy steps per env on a zero fp64 table, explore streams seeded anew,
      one launch, kernel time from the handle's HIP-event timing;
  (b) envs_rollout_kernel on a uniform-random time-indexed policy over the first n_act lanes (drawn once, on
      the device): the parent's kernel and the yardstick.  It stops an env that terminates, so it takes fewer
      env-steps than (a), which restarts it; each side's time is divided by its own env-steps.
Workloads: FourRooms x 4096, LavaCrossingS11N5 x 65536, and the latter with NoDeath lava on the handle (see
WORKLOADS).  The sides alternate inside every repetition; medians over the repetitions with min-max.  Every
repetition of (a) must reproduce the first one's table and returns, and leave the envs as loaded; every
repetition of (b) the first one's steps and returns (asserted).  One JSON line per workload; --out appends them
to a file.

    python tools/probe_qlearn.py [--out profiles/qlearn/probe_qlearn.jsonl] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (env id, B, NoDeath lava).  On lava grids (b) stops an env at its first lava cell while the wave runs on, so
# its time per env-step counts idle lanes; with NoDeath(("lava",)) on the handle lava costs and the episode
# goes on, and both sides take n_steps steps per env.
WORKLOADS = [("MiniGrid-FourRooms-v0", 4096, False), ("MiniGrid-LavaCrossingS11N5-v0", 65536, False),
             ("MiniGrid-LavaCrossingS11N5-v0", 65536, True)]


def stats(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=256)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--n-act", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    args = ap.parse_args()
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen
    from minigrid_dynamicprogramming_amd.dp import n_actions, n_states

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    dev = torch.device("cuda", 0)
    model, n, n_act = "xyd", args.n_steps, args.n_act
    for env_id, B, nodeath in WORKLOADS:
        B = max(1, int(B * args.scale))
        g = gen.generate(env_id, 0, B)
        enc, agent = g["enc"], g["agent"]
        venv = mg.MiniGridVecEnv(env_id, B, no_death_types=("lava",) if nodeath else ())
        S, A = n_states(model, venv.W, venv.H), n_actions(model)
        gen_t = torch.Generator(device=dev).manual_seed(args.seed)
        pi = torch.randint(0, n_act, (n, B, S), dtype=torch.int8, device=dev, generator=gen_t)
        Q = torch.zeros((B, S, A), dtype=torch.float64, device=dev)
        steps, episodes, wins, status = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
        ret = torch.zeros(B, dtype=torch.float64, device=dev)
        term = torch.zeros(B, dtype=torch.uint8, device=dev)
        trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        venv.load(enc, agent, max_steps=n)
        loaded = venv.get_state()
        venv.enable_timing(True)

        def learn():
            Q.zero_()
            torch.cuda.synchronize()
            venv.set_explore(args.seed)
            ms0, n0 = venv.kernel_time()
            venv.q_learn_device(Q, n, model, steps, episodes, wins, ret, status, eps=args.eps, n_act=n_act)
            ms1, n1 = venv.kernel_time()
            assert n1 - n0 == 1
            torch.cuda.synchronize()
            return (ms1 - ms0) * 1e3, float(Q.sum().item()), ret.cpu().numpy().copy()

        def rollout():
            ms0, n0 = venv.kernel_time()
            venv.rollout_device(pi, n, model, n, steps, ret, term, trunc, status)
            ms1, n1 = venv.kernel_time()
            assert n1 - n0 == 1
            torch.cuda.synchronize()
            out = (ms1 - ms0) * 1e3, steps.cpu().numpy().copy(), ret.cpu().numpy().copy()
            venv.load(enc, agent, max_steps=n)  # the rollout moved the envs
            return out

        _, q_sum, q_ret = learn()  # also the warm-up of (a)
        assert (status.cpu().numpy() == 0).all() and (steps.cpu().numpy() == n).all()
        q_episodes, q_wins = int(episodes.sum().item()), int(wins.sum().item())
        after = venv.get_state()
        assert all(np.array_equal(after[k], loaded[k]) for k in loaded), "q_learn changed an env"
        _, r_steps, r_ret = rollout()
        assert (status.cpu().numpy() == 0).all()
        times = {"a": [], "b": []}
        for _ in range(args.reps):
            t, s, r = learn()
            assert s == q_sum and np.array_equal(r, q_ret)
            times["a"].append(t)
            t, s, r = rollout()
            assert np.array_equal(s, r_steps) and np.array_equal(r, r_ret)
            times["b"].append(t)
        venv.close()
        a, b = stats(times["a"]), stats(times["b"])
        a_steps, b_steps = B * n, int(r_steps.sum())
        a_step, b_step = a["median"] / a_steps, b["median"] / b_steps
        rec = {"env": env_id, "B": B, "nodeath_lava": nodeath, "model": model, "box": box, "reps": args.reps,
               "n_steps": n, "eps": args.eps, "n_act": n_act, "seed": args.seed, "S": S, "q_table_bytes": B * S * A * 8,
               "a_qlearn_kernel_us": a, "a_env_steps": a_steps, "a_episodes": q_episodes, "a_wins": q_wins,
               "a_env_steps_per_s": round(a_steps / (a["median"] * 1e-6), 1),
               "b_rollout_kernel_us": b, "b_env_steps": b_steps, "b_mean_steps_per_env": round(b_steps / B, 2),
               "b_env_steps_per_s": round(b_steps / (b["median"] * 1e-6), 1),
               "a_kernel_ns_per_env_step": round(a_step * 1e3, 4), "b_kernel_ns_per_env_step": round(b_step * 1e3, 4),
               "a_over_b_per_env_step": round(a_step / b_step, 3)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del pi, Q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
