"""Measurement on the MI355X for job priorities in a queue session (dsg_queue_set_priority / _park / _resume): what a priority buys a
live speaker who arrives while every slot holds a batch clip, and what a park and a resume cost a round.  ZEGGS dims, bf16, one lane,
B = 16, the 1000-step DDPM (`--skip` for a rehearsal at fewer steps), sixteen closed jobs of K = 8 at priority 0.
  (1) After two rounds a live job with one window is submitted.  The wall time from the call of `submit_live` until that window's rows
      are in the caller's host memory, once with the live job at priority 1 (it takes the slot of a batch clip, which is parked) and once
      at priority 0 (it waits until the batch clips end), with the rounds it took.
  (2) The wall time of `run(1)` for a round in which one job is parked and one resumed (`park` on a running job, `resume` on the one
      parked the round before, which takes the slot that one left: sixteen slots run) against a round of the same session without
      either, next to `dsg_last_sample_ms`, the step loop alone.
Synthetic state dict and features: nothing outside the repository is read.  One JSON line at the end; nothing is asserted about a time.

    python tools/queue_priority_latency.py [--skip 0] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, K_BATCH = 16, 8


def main():
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd import lib as L
    from diffusestylegesture_amd import sample as S
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    p = argparse.ArgumentParser()
    p.add_argument("--skip", type=int, default=0)
    p.add_argument("--rounds", type=int, default=3, help="rounds timed with and without a park + resume")
    args = p.parse_args()
    cfg = C.ZEGGS
    m = DSGDenoiser(cfg, precision="bf16", max_batch=B, device=0)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    d = create_gaussian_diffusion()
    style = np.eye(cfg.style_dim_in, dtype=np.float32)[0]

    def batch(K, n=B):
        return [{"feats": [synth_window_inputs(cfg, 1, window=w, clips=[c])["audio"] for w in range(K)], "style": style, "clip_id": c}
                for c in range(n)]

    def timed_round(q):
        t0 = time.perf_counter()
        n = q.run(1)
        t1 = time.perf_counter()
        assert n == 1
        return 1e3 * (t1 - t0), float(m.last_sample_ms()[0])

    open_queue = lambda: S.open_clip_queue(m, d, seed=123456, skip_timesteps=args.skip, kernel_set=None, B=B)
    jobs = batch(K_BATCH)
    live_feats = synth_window_inputs(cfg, 1, window=0, clips=[B])["audio"]
    out = {"what": "ZEGGS bf16, one lane, B=16, sixteen closed jobs of K=8 at priority 0", "steps": d.num_timesteps - args.skip}
    # (1) a live job arrives after two rounds
    for prio in (1, 0):
        with open_queue() as q:
            tickets = [q.submit(j) for j in jobs]
            assert q.run(2) == 2
            t0 = time.perf_counter()
            lv = q.submit_live({"feats": [live_feats], "style": style, "clip_id": B}, 2, priority=prio)
            rounds, per = 0, []
            while q.job(lv)["rows_ready"] == 0:
                per.append(timed_round(q)[0])
                rounds += 1
            t1 = time.perf_counter()
            assert q.job(lv)["rows_ready"] == cfg.stride - cfg.n_seed and np.isfinite(q.rows(lv)).all()
            out[f"live_priority_{prio}"] = {"submit_to_rows_ms": 1e3 * (t1 - t0), "rounds": rounds, "round_ms": per,
                                            "batch_jobs_parked": sum(q.job(t)["parks"] for t in tickets)}
            kset, path = m.last_kernel_set(), m.last_sample_path()
    # (2) a round with one park and one resume against a round without
    with open_queue() as q:
        tickets = [q.submit(j) for j in batch(2 * args.rounds + 4, B + 1)]      # seventeen jobs: sixteen run, one waits
        assert q.run(2) == 2                                   # warm-up
        plain = [timed_round(q) for _ in range(args.rounds)]
        q.park(tickets[0])                                     # it leaves and the waiting job takes its slot on window 0: not timed
        assert q.run(1) == 1 and q.job(tickets[0])["state"] == L.JOB_PARKED and q.job(tickets[B])["state"] == L.JOB_RUNNING
        moved = []
        for r in range(args.rounds):
            q.resume(tickets[r])
            q.park(tickets[r + 1])
            moved.append(timed_round(q))
            assert q.job(tickets[r])["state"] == L.JOB_RUNNING and q.job(tickets[r + 1])["state"] == L.JOB_PARKED
            assert q.queue.info()["n_running"] == B
        assert sum(q.job(t)["parks"] for t in tickets) == args.rounds + 1
    med = statistics.median
    out["round_plain"] = {"run_ms": {"median": med(a for a, _ in plain), "all": [a for a, _ in plain]},
                          "last_sample_ms": {"median": med(b for _, b in plain)}}
    out["round_park_resume"] = {"run_ms": {"median": med(a for a, _ in moved), "all": [a for a, _ in moved]},
                                "last_sample_ms": {"median": med(b for _, b in moved)}}
    out["park_resume_adds_ms"] = out["round_park_resume"]["run_ms"]["median"] - out["round_plain"]["run_ms"]["median"]
    out["kernel_set"], out["path"] = kset, path
    print(json.dumps(out))


if __name__ == "__main__":
    main()
