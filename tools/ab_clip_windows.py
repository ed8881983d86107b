"""A/B on the MI355X: the host window loop (`windows="host"`: one library call per window, hand-off and stitching in torch) against the whole
clip in one library call (`windows="library"`: dsg_sample_clip, k_window_handoff), in ONE process on ONE handle per workload, in
interleaved rounds (host, library, host, ...) after a warm-up of both.  Per workload it prints wall time per pass (host clock around a
call that ends in a device synchronise: both forms return host memory) and the library's summed step-loop time (dsg_last_sample_ms),
each as median and min .. max over the rounds, the spread of the host form standing for the run-to-run noise, and whether the two
outputs of the last round are bit-identical.  One JSON line per workload at the end.

    python tools/ab_clip_windows.py [--rounds 5] [--workloads config2,headline,config3] [--skip 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {
    # name: (sampler, lanes, clips per lane, windows)
    "config2": ("ddim50", 1, 16, 4),        # DDIM-50, 16 clips in lock step, 4 windows
    "headline": ("ddpm", 1, 1, 4),          # 1 clip, 4 x 1000 DDPM steps
    "config3": ("ddpm", 4, 4, 4),           # 4 lanes x 4 clips, 4 x 1000 DDPM steps
}


def main():
    import torch
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.sample import generate_clip, generate_clips_streams
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--workloads", default="config2,headline,config3")
    p.add_argument("--skip", type=int, default=0, help="skip_timesteps (a rehearsal at fewer steps; 0 = the workloads as named)")
    args = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    cfg = C.ZEGGS
    sd = synth_state_dict(cfg, 20240)
    style = [1, 0, 0, 0, 0, 0]
    for name in args.workloads.split(","):
        sampler, NL, B, K = WORKLOADS[name]
        ddim = sampler == "ddim50"
        d = create_gaussian_diffusion("ddim50" if ddim else "")
        m = DSGDenoiser(cfg, precision="bf16", max_batch=B, device=0)
        m.load_state_dict(sd)
        lanes = [m] + [m.clone() for _ in range(NL - 1)]
        feats = [[torch.from_numpy(synth_window_inputs(cfg, B, window=w, clip0=ln * B)["audio"]).cuda() for w in range(K)] for ln in range(NL)]
        acc = {"ms": 0.0}
        # the host loop's step time: summed per window (every window is one library call whose time the next one overwrites)
        orig_multi, orig_single = d.p_sample_loop_multi, d.p_sample_loop
        orig_ddim = d.ddim_sample_loop

        def timed(fn):
            def w(*a, **k):
                out = fn(*a, **k)
                acc["ms"] += max(ln.last_sample_ms()[0] for ln in lanes)
                return out
            return w
        d.p_sample_loop_multi, d.p_sample_loop, d.ddim_sample_loop = timed(orig_multi), timed(orig_single), timed(orig_ddim)

        def run(windows):
            acc["ms"] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if NL > 1:
                out = generate_clips_streams(lanes, d, feats, style, seed=123456, skip_timesteps=args.skip, ddim=ddim, windows=windows)
            else:
                out = generate_clip(m, d, feats[0], style, seed=123456, skip_timesteps=args.skip, ddim=ddim, windows=windows)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            steps = acc["ms"] if windows == "host" else max(ln.last_sample_ms()[0] for ln in lanes)
            return wall, steps, out
        for w in ("host", "library"):          # warm-up of both forms: code objects, buffers, the AQL plan
            run(w)
        res = {"host": [], "library": []}
        outs = {}
        for r in range(args.rounds):
            for w in ("host", "library"):
                wall, steps, outs[w] = run(w)
                res[w].append((wall, steps))
                print(f"{name} round {r} {w:8s} wall {wall:10.3f} ms   step loops {steps:10.3f} ms   outside the step loops {wall - steps:8.3f} ms", flush=True)
        rec = {"workload": name, "sampler": sampler, "lanes": NL, "clips_per_lane": B, "windows": K, "rounds": args.rounds,
               "skip_timesteps": args.skip, "kernel_set": lanes[0].last_kernel_set(), "path": lanes[0].last_sample_path(),
               "bit_identical": bool(np.array_equal(outs["host"], outs["library"]))}
        for w in ("host", "library"):
            walls, steps = [a for a, _ in res[w]], [b for _, b in res[w]]
            rec[w] = {"wall_ms_median": statistics.median(walls), "wall_ms_min": min(walls), "wall_ms_max": max(walls),
                      "step_ms_median": statistics.median(steps), "step_ms_min": min(steps), "step_ms_max": max(steps)}
        rec["wall_gain_pct"] = 100.0 * (1.0 - rec["library"]["wall_ms_median"] / rec["host"]["wall_ms_median"])
        rec["host_spread_pct"] = 100.0 * (rec["host"]["wall_ms_max"] - rec["host"]["wall_ms_min"]) / rec["host"]["wall_ms_median"]
        print(json.dumps(rec), flush=True)
        del lanes, m


if __name__ == "__main__":
    main()
