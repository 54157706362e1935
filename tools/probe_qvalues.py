"""The action-value read-out beside the improvement step on one handle: microseconds of

    a   action_values_device(Q, opt)     vi_qvalues_kernel, Q and opt written
    b   action_values_device(None, opt)  vi_qvalues_kernel, opt only (no staging, no Q)
    c   improve()                        vi_improve_kernel: the same V and cells read, the same Q computed, pi written

on a solved handle.  a and b are timed by the handle's HIP events (kernel_time: the dispatch's own begin and end).
improve()'s launch carries no event pair, so every side is also timed by an event pair recorded on the handle's
stream around the whole call (`*_call_us`: the launch plus what the call enqueues around it -- improve() an
8-byte memset and an 8-byte copy -- and the gaps between them); a's and b's `call - kernel` differences show what
that adds.  The sides alternate within a repetition after a warm-up call of each; the figure is the median of
--reps repetitions with min-max.  `floor_us`: the bytes a moves (Q written, V and cells read) at 6.0-6.3 TB/s.
One JSON line per workload; --out appends them to a file.

    python tools/probe_qvalues.py [--out profiles/qvalues/probe_qvalues.jsonl] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [("MiniGrid-LavaCrossingS11N5-v0", 65536, "xyd"),
             ("MiniGrid-FourRooms-v0", 4096, "xyd"),
             ("MiniGrid-DoorKey-16x16-v0", 4096, "doorkey")]
SIDES = ("a", "b", "c")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (rehearsals)")
    ap.add_argument("--only", type=int, default=-1, help="run one workload by index")
    args = ap.parse_args()
    import torch

    import minigrid_dynamicprogramming_amd as mg
    from minigrid_dynamicprogramming_amd import _lib, gen
    from minigrid_dynamicprogramming_amd.dp import n_actions

    _lib.pin_host_thread(0)
    box = torch.cuda.get_device_name(0)
    tdt = torch.float32 if args.dtype == "f32" else torch.float64
    tsize = 4 if args.dtype == "f32" else 8
    for i, (env, B, model) in enumerate(WORKLOADS):
        if args.only >= 0 and i != args.only:
            continue
        B = max(1, int(B * args.scale))
        cells = gen.generate(env, 0, B, enc=False, cells=True, agent=False)["cells"]
        stream = torch.cuda.Stream()
        vi = mg.ValueIteration(cells, model=model, dtype=args.dtype, stream=stream.cuda_stream)
        vi.solve()
        A = n_actions(model)
        Q = torch.empty((B, vi.S, A), dtype=tdt, device="cuda")
        opt = torch.empty((B, vi.S), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        calls = {"a": lambda: vi.action_values_device(Q.data_ptr(), opt.data_ptr()),
                 "b": lambda: vi.action_values_device(None, opt.data_ptr()),
                 "c": lambda: vi.improve()}
        # warm-up, and the check that the three sides agree: after a solve with dV = 0 improve() changes nothing
        # (pi* holds a maximising lane everywhere) and the opt-only launch writes the same sets
        calls["a"]()
        opt_a = opt.clone()
        calls["b"]()
        assert torch.equal(opt, opt_a)
        changed = calls["c"]()
        assert vi.dv != 0.0 or changed == 0, changed
        assert bool(vi.is_optimal(vi.policy()).all()) or vi.dv != 0.0
        vi.enable_timing(True)
        kern = {s: [] for s in SIDES}
        call = {s: [] for s in SIDES}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.reps):
            for s in SIDES:  # alternating: every side sees the same clocks and neighbours
                ms0, _ = vi.kernel_time()
                e0.record(stream)
                calls[s]()
                e1.record(stream)
                e1.synchronize()
                ms1, _ = vi.kernel_time()
                kern[s].append((ms1 - ms0) * 1e3)
                call[s].append(e0.elapsed_time(e1) * 1e3)
        q_bytes = B * vi.S * A * tsize
        in_bytes = B * vi.S * tsize + cells.size
        rec = {"env": env, "B": B, "model": model, "dtype": args.dtype, "box": box, "lib": os.path.basename(_lib.lib_path()),
               "reps": args.reps, "q_bytes": q_bytes, "v_and_cells_bytes": in_bytes,
               "floor_us": [round((q_bytes + in_bytes) / 6.3e12 * 1e6, 1), round((q_bytes + in_bytes) / 6.0e12 * 1e6, 1)]}
        for s in SIDES:
            if s != "c":  # improve()'s launch is not on the handle's events
                rec[f"{s}_kernel_us"] = round(float(np.median(kern[s])), 1)
                rec[f"{s}_kernel_us_min_max"] = [round(min(kern[s]), 1), round(max(kern[s]), 1)]
            rec[f"{s}_call_us"] = round(float(np.median(call[s])), 1)
            rec[f"{s}_call_us_min_max"] = [round(min(call[s]), 1), round(max(call[s]), 1)]
        rec["a_kernel_over_floor"] = round(rec["a_kernel_us"] / rec["floor_us"][1], 2)
        rec["a_write_TBps"] = round(q_bytes / rec["a_kernel_us"] / 1e6, 2)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        vi.close()
        del Q, opt, opt_a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
