"""Measurement on the MI355X for live jobs of a queue session (dsg_queue_submit_live / _append): what the session adds per window.
One live job alone -- ZEGGS dims, bf16, one lane, B = 1, the 1000-step DDPM (`--skip` for a rehearsal at fewer steps) -- is fed one
window per round.  Per window: the wall time from the call of `append` (a host window: staged by the call) until the window's rows are in
the caller's host memory (`run(1)` has returned), next to `dsg_last_sample_ms` of that round, the step loop alone.  The difference is the
session's: staging the window, the round's tables and gather, the hand-off, the row copy and its synchronisation.  Synthetic state dict and
features: nothing outside the repository is read.  One JSON line at the end.

    python tools/live_latency.py [--windows 6] [--skip 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd import sample as S
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=6, help="windows fed after the warm-up window")
    p.add_argument("--skip", type=int, default=0)
    args = p.parse_args()
    cfg = C.ZEGGS
    m = DSGDenoiser(cfg, precision="bf16", max_batch=1, device=0)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    d = create_gaussian_diffusion()
    feats = [synth_window_inputs(cfg, 1, window=w, clips=[0])["audio"] for w in range(args.windows + 1)]
    style = np.eye(cfg.style_dim_in, dtype=np.float32)[0]
    wall, loop = [], []
    with S.open_clip_queue(m, d, seed=123456, skip_timesteps=args.skip, kernel_set=None, B=1) as q:
        t = q.submit_live({"feats": [feats[0]], "style": style, "clip_id": 0}, args.windows + 1)
        assert q.run(1) == 1                                  # warm-up: the first window
        rows = q.job(t)["rows_ready"]
        for w in range(1, args.windows + 1):
            t0 = time.perf_counter()
            q.append(t, feats[w], last=w == args.windows)
            n = q.run(1)
            t1 = time.perf_counter()
            assert n == 1 and q.job(t)["rows_ready"] > rows
            rows = q.job(t)["rows_ready"]
            wall.append(1e3 * (t1 - t0))
            loop.append(float(m.last_sample_ms()[0]))
        clip = q.result(t)
        path, kset = m.last_sample_path(), m.last_kernel_set()
    assert np.isfinite(clip).all() and clip.shape == ((args.windows + 1) * cfg.stride - cfg.n_seed, cfg.njoints)
    added = [a - b for a, b in zip(wall, loop)]
    med = statistics.median
    print(json.dumps({"what": "live job alone, ZEGGS bf16 B=1, per window", "steps": d.num_timesteps - args.skip, "windows": args.windows,
                      "kernel_set": kset, "path": path,
                      "append_to_rows_ms": {"median": med(wall), "min": min(wall), "max": max(wall)},
                      "last_sample_ms": {"median": med(loop), "min": min(loop), "max": max(loop)},
                      "session_adds_ms": {"median": med(added), "min": min(added), "max": max(added)}}))


if __name__ == "__main__":
    main()
