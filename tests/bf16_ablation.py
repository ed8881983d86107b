#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (a study, not a collected test): where does the bf16 drift of the headline configuration come from?

The HIP bf16 path rounds to bf16 at a fixed list of points (operands of the MFMA contractions; everything else -- residual stream,
LayerNorm statistics, local attention, conditioning, the sampler update -- is fp32).  This script restates the fp32 numpy oracle
with a switch per rounding point (round-to-nearest-even to 8 mantissa bits, products / sums in fp32 like the MFMA), runs a whole
1000-step DDPM window of the headline workload (ZEGGS, batch 1, the Philox noise of the goldens) per variant and reports the
relative L2 distance to the pure fp32 oracle:

    python tests/bf16_ablation.py [--steps 1000] [--windows 1] [--only] [--except]

  all          every point on  (= what the HIP bf16 path does; cross-checked on the GPU: tests/test_gpu_round4.py)
  only:<p>     only point p on
  except:<p>   every point but p

Points: weights (all packed matrices), state (x_t as the pose embedding's operand), x0a (encoder input into the layer-0 QKV), ln2
(LayerNorm2 rows into QKV / the pose head), qk (Q and K as stored), v (V as stored), p (softmax numerators into the PV product),
attn (attention rows into out_proj), ln1 (LayerNorm1 rows into linear1), hidden (GELU output into linear2).
The switchable oracle itself is oracle/rounded.py (tests/rowcheck.py bounds every row of a device result with it).
Result of the run behind DESIGN.md s2 (round 4): profiles/r04_bf16_ablation_oracle.log."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffusestylegesture_amd import config as C                       # noqa: E402
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs      # noqa: E402
from oracle import sampler                                           # noqa: E402
from oracle.rounded import POINTS, WPOINTS, RoundedOracle, bf16     # noqa: E402,F401
from oracle.schedule import OracleDiffusion                          # noqa: E402


def run(on, sd, cfg, steps, windows, seed):
    m = RoundedOracle(sd, cfg, on, device_form=True)      # the fp32 baseline in the library's form too (folded embedding)
    d = OracleDiffusion()
    shape = (1, cfg.njoints, 1, cfg.n_poses)
    outs, prev = [], None
    for w in range(windows):
        y = synth_window_inputs(cfg, 1, window=w)
        if prev is not None:
            y["seed"] = prev[..., -cfg.n_seed:]
        base = w * (1 + steps)                                    # one Philox stream runs through the windows of a clip
        nf = (lambda b: (lambda dr: sampler.philox.normal_bj1t(shape, seed, b + dr, 0)))(base)
        prev = sampler.p_sample_loop(d, m, shape, nf, {"y": y}, skip_timesteps=1000 - steps)
        outs.append(prev)
    return np.concatenate(outs, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--seed", type=int, default=123456)
    ap.add_argument("--modes", default="all,only,except")
    a = ap.parse_args()
    cfg = C.ZEGGS
    sd = synth_state_dict(cfg, 20240)
    from threadpoolctl import threadpool_limits
    rel = lambda x, r: float(np.linalg.norm(x.astype(np.float64) - r) / np.linalg.norm(r))
    with threadpool_limits(limits=8):
        t0 = time.time()
        ref = run([], sd, cfg, a.steps, a.windows, a.seed).astype(np.float64)
        print(f"fp32 oracle: {a.windows} window(s) x {a.steps} steps in {time.time() - t0:.1f} s", flush=True)
        variants = []
        if "all" in a.modes:
            variants.append(("all", POINTS))
        if "only" in a.modes:
            variants += [("only:" + p, [p]) for p in POINTS]
        if "wsplit" in a.modes:
            variants += [("only:" + p, [p]) for p in WPOINTS] + [("all-but-weights", [q for q in POINTS if q != "weights"]),
                                                                 ("all, w_out+w_in fp32", [q for q in POINTS if q != "weights"] + ["w_qkv", "w_o", "w_1", "w_2"]),
                                                                 ("all, w_1+w_2 fp32", [q for q in POINTS if q != "weights"] + ["w_qkv", "w_o", "w_in", "w_out"])]
        if "except" in a.modes:
            variants += [("except:" + p, [q for q in POINTS if q != p]) for p in POINTS]
        for name, on in variants:
            out = run(on, sd, cfg, a.steps, a.windows, a.seed)
            print(f"{name:16s} rel-L2 vs fp32 oracle = {rel(out, ref):.3e}", flush=True)


if __name__ == "__main__":
    main()
