"""Measurement on the MI355X for the clip queue (dsg_sample_clip_queue): a synthetic corpus of 48 clips of different lengths (269 windows in
all), ZEGGS dims, bf16, one lane, 16 slots.  Synthetic state dict and features: nothing outside the repository is read.

(a) the corpus through `generate_clip_queue` (17 rounds = ceil(269 / 16)) against the best the lock-step API can do: groups of 16 clips
    sorted by length, the short ones padded with zero-feature windows whose frames are thrown away, through
    `generate_clip(windows="library", clip_ids=...)` (23 rounds).  Wall time per whole corpus (host clock around calls that end in host
    memory), warm, `--rounds` repeats, with DDIM-50 and the 1000-step DDPM.  `--baseline-only` runs on a checkout without the queue.
(b) the price of the per-element draw offset in the pose head: `last_step_time_us` of a keyed 16-clip ROWS call (`clip_streams=`), a warm-up
    and four repeats of a 200-step loop.  Run it on two builds (DSG_LIB=...) in one session and compare.

(c) the queue as a session (dsg_queue_*, `sample.open_clip_queue`) against the one-shot `generate_clip_queue`, with the corpus as host
    tensors and as device tensors: wall time per corpus (the session: all 48 clips submitted longest first, then `run(1)` until idle);
    the gap between two step loops per round (the session: wall of `run(1)` minus `last_sample_ms`; the one-shot call: wall minus
    `last_sample_ms`, over its 17 rounds); and the time from `submit` until `rows_ready > 0` for a clip that arrives after round 3 of the
    other 47 -- behind 47 clips in index order (ticket 47, first come first served) and behind 47 clips submitted longest first -- beside
    the time the one-shot call still has to run at that moment (14 of its 17 rounds).  `--oneshot-only` measures the one-shot side alone:
    that is how the parent commit is measured (this file run in a checkout of the parent, in the same sitting); without it part (c)
    measures the session alone, one session kept open over the warm-up and every repeat.

One JSON line at the end.

    python tools/clip_queue_bench.py [--rounds 5] [--samplers ddim50,ddpm] [--parts a,b,c] [--baseline-only] [--oneshot-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K48 = [4, 2, 5, 16, 1, 2, 8, 2, 4, 12, 1, 8, 3, 1, 2, 5, 5, 2, 3, 2, 8, 5, 1, 12, 2, 3, 16, 16, 12, 1, 12, 12, 5, 1, 3, 1, 8, 2, 3, 5, 2, 8, 2, 12, 3,
       8, 16, 2]
SLOTS = 16


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def part_c(args, cfg, m, style):
    import torch
    from diffusestylegesture_amd import sample as S
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.synth import synth_window_inputs
    host = [[synth_window_inputs(cfg, 1, window=w, clips=[i])["audio"] for w in range(K)] for i, K in enumerate(K48)]
    corpus = {"host": host, "device": [[torch.from_numpy(f).cuda() for f in fs] for fs in host]}
    longest_first = sorted(range(len(K48)), key=lambda i: -K48[i])
    out = {}
    for sampler in args.samplers.split(","):
        ddim = sampler == "ddim50"
        d = create_gaussian_diffusion("ddim50" if ddim else "")
        kw = dict(seed=123456, skip_timesteps=args.skip, ddim=ddim, kernel_set=None, B=SLOTS)
        a = {"skip_timesteps": args.skip}
        results = {}
        for kind, feats in corpus.items():
            clips = [{"feats": f, "style": style, "clip_id": i} for i, f in enumerate(feats)]

            def oneshot():
                got = S.generate_clip_queue(m, d, clips, **kw)
                step_ms = m.last_sample_ms()[0]
                return got, step_ms, None

            # one session for the warm-up and every repeat, as a service keeps it: its staging is recycled from the second corpus on
            q = None if args.oneshot_only else S.open_clip_queue(m, d, **kw)
            submit_ms = []

            def session():
                gaps, step_ms = [], 0.0
                t0 = time.perf_counter()
                tickets = {i: q.submit(clips[i]) for i in longest_first}
                submit_ms.append((time.perf_counter() - t0) * 1e3)
                while True:
                    t0 = time.perf_counter()
                    n = q.run(1)
                    wall = (time.perf_counter() - t0) * 1e3
                    if n == 0:
                        break
                    ms = m.last_sample_ms()[0]
                    gaps.append(wall - ms)
                    step_ms += ms
                got = [q.result(tickets[i]) for i in range(len(clips))]
                return got, step_ms, gaps
            forms = {"oneshot": oneshot} if args.oneshot_only else {"session": session}
            res = {k: [] for k in forms}
            for r in range(-1, args.rounds):
                for name, fn in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    results[kind, name], step_ms, gaps = fn()
                    torch.cuda.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    gap = (wall - step_ms) / 17.0 if gaps is None else statistics.median(gaps)
                    if r >= 0:
                        res[name].append((wall, step_ms, gap))
                    print(f"(c) {sampler} {kind:6s} round {r} {name:8s} wall {wall:10.3f} ms   step loops {step_ms:10.3f} ms   gap per round {gap:7.3f} ms"
                          + ("" if gaps is None else f"   rounds {len(gaps)}"), flush=True)
            if q is not None:
                q.close()
            a[kind] = {name: {"wall_ms": _stats([w for w, _, _ in v]), "step_ms": _stats([s for _, s, _ in v]),
                              "gap_per_round_ms": _stats([g for _, _, g in v])} for name, v in res.items()}
            if submit_ms:
                a[kind]["session"]["submit_48_ms"] = _stats(submit_ms[1:])
        a["kernel_set"], a["path"] = m.last_kernel_set(), m.last_sample_path()
        first = next(iter(results.values()))
        a["bit_identical"] = bool(all(np.array_equal(x, y) for k in results for x, y in zip(results[k], first)))
        if not args.oneshot_only:
            # a request that arrives after round 3 of the other 47 clips: the time until its first window is in the caller's memory
            clips = [{"feats": f, "style": style, "clip_id": i} for i, f in enumerate(corpus["host"])]
            late = {}
            for order_name, order in (("fifo_index_order", list(range(47))), ("longest_first", [i for i in longest_first if i != 47])):
                ms, waited = [], []
                for r in range(-1, args.rounds):
                    with S.open_clip_queue(m, d, **kw) as q:
                        for i in order:
                            q.submit(clips[i])
                        assert q.run(3) == 3
                        t0 = time.perf_counter()
                        t = q.submit(clips[47])
                        n = 0
                        while q.job(t)["rows_ready"] == 0:
                            assert q.run(1) == 1
                            n += 1
                        if r >= 0:
                            ms.append((time.perf_counter() - t0) * 1e3)
                            waited.append(n)
                        first_round = q.job(t)["first_round"]
                    print(f"(c) {sampler} late request, {order_name}: first window after {n} rounds (its window 0 in session round {first_round})", flush=True)
                late[order_name] = {"first_window_ms": _stats(ms), "rounds_waited": waited[0], "first_round": first_round}
            late["corpus_rounds_still_to_run"] = 14
            a["late_request"] = late
        out[sampler] = a
    return out


def main():
    import torch
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd import sample as S
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--samplers", default="ddim50,ddpm")
    p.add_argument("--parts", default="a,b")
    p.add_argument("--baseline-only", action="store_true", help="part (a): only the lock-step baseline (runs without the queue API)")
    p.add_argument("--oneshot-only", action="store_true", help="part (c): only the one-shot call (runs without the session API)")
    p.add_argument("--skip", type=int, default=0, help="skip_timesteps of parts (a) and (c) (a rehearsal at fewer steps)")
    args = p.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    assert sum(K48) == 269 and len(K48) == 48
    cfg = C.ZEGGS
    T, S_, J = cfg.n_poses, cfg.n_seed, cfg.njoints
    sd = synth_state_dict(cfg, 20240)
    m = DSGDenoiser(cfg, precision="bf16", max_batch=SLOTS, device=0)
    m.load_state_dict(sd)
    rec = {"tool": "clip_queue_bench", "lib": os.path.basename(m.lib.path), "slots": SLOTS, "clips": len(K48), "windows": sum(K48)}
    style = np.array([1, 0, 0, 0, 0, 0], np.float32)
    if "a" in args.parts.split(","):
        feats = [[torch.from_numpy(synth_window_inputs(cfg, 1, window=w, clips=[i])["audio"]).cuda() for w in range(K)] for i, K in enumerate(K48)]
        zero = torch.zeros_like(feats[0][0])
        # the baseline's groups: sorted by length (longest first), 16 at a time, padded to the group's longest
        order = sorted(range(len(K48)), key=lambda i: -K48[i])
        groups = [order[g:g + SLOTS] for g in range(0, len(order), SLOTS)]
        base_rounds = sum(K48[g[0]] for g in groups)
        g_feats = [[torch.cat([feats[i][w] if w < K48[i] else zero for i in g]) for w in range(K48[g[0]])] for g in groups]
        sty16 = np.repeat(style[None], SLOTS, 0)
        rec["baseline_rounds"] = base_rounds
        assert base_rounds == 23
        if not args.baseline_only:
            from diffusestylegesture_amd import lib as L
            rec["queue_rounds"] = L.clip_queue_plan(K48, SLOTS, m.lib)[2]
            assert rec["queue_rounds"] == 17
            clips = [{"feats": f, "style": style, "clip_id": i} for i, f in enumerate(feats)]
        for sampler in args.samplers.split(","):
            ddim = sampler == "ddim50"
            d = create_gaussian_diffusion("ddim50" if ddim else "")

            def baseline():
                out = [None] * len(K48)
                step_ms = 0.0
                for g, gf in zip(groups, g_feats):
                    seq = S.generate_clip(m, d, gf, sty16[:len(g)], seed=123456, skip_timesteps=args.skip, ddim=ddim, windows="library", clip_ids=g)
                    step_ms += m.last_sample_ms()[0]
                    for b, i in enumerate(g):
                        out[i] = seq[b, :K48[i] * (T - S_) - S_]
                return out, step_ms

            def queue():
                out = S.generate_clip_queue(m, d, clips, seed=123456, skip_timesteps=args.skip, ddim=ddim, kernel_set=None, B=SLOTS)
                return out, m.last_sample_ms()[0]
            forms = {"baseline": baseline} if args.baseline_only else {"baseline": baseline, "queue": queue}
            res = {k: [] for k in forms}
            outs = {}
            for r in range(-1, args.rounds):          # round -1: warm-up of every form (code objects, buffers, the AQL plan)
                for name, fn in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[name], step_ms = fn()
                    torch.cuda.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    if r >= 0:
                        res[name].append((wall, step_ms))
                    print(f"{sampler} round {r} {name:8s} wall {wall:10.3f} ms   step loops {step_ms:10.3f} ms   outside {wall - step_ms:8.3f} ms", flush=True)
            a = {"kernel_set": m.last_kernel_set(), "path": m.last_sample_path(), "skip_timesteps": args.skip}
            for name in forms:
                a[name] = {"wall_ms": _stats([w for w, _ in res[name]]), "step_ms": _stats([s for _, s in res[name]])}
            b = a["baseline"]["wall_ms"]
            a["baseline_spread_pct"] = 100.0 * (b["max"] - b["min"]) / b["median"]
            if "queue" in forms:
                a["speedup_wall"] = b["median"] / a["queue"]["wall_ms"]["median"]
                a["speedup_steps"] = a["baseline"]["step_ms"]["median"] / a["queue"]["step_ms"]["median"]
                a["predicted"] = 23.0 / 17.0
                # the same clip -> motion map: a padded clip's frames up to its own length are the clip's (rows are independent)
                a["bit_identical"] = bool(all(np.array_equal(x, y) for x, y in zip(outs["baseline"], outs["queue"])))
            rec[sampler] = a
    if "c" in args.parts.split(","):
        rec["c"] = part_c(args, cfg, m, style)
    if "b" in args.parts.split(","):
        d = create_gaussian_diffusion("")
        m.set_kernel_set("rows")
        y = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in synth_window_inputs(cfg, SLOTS, window=0).items()}
        us = []
        for r in range(-1, 4):
            d.manual_seed(123456, 0).p_sample_loop(m, (SLOTS, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=800,
                                                   clip_streams=list(range(SLOTS)))
            if r >= 0:
                us.append(d.last_step_time_us())
            print(f"keyed rows 16 clips, 200 steps, repeat {r}: {d.last_step_time_us():.2f} us/step", flush=True)
        rec["keyed_rows16_us_per_step"] = dict(_stats(us), kernel_set=m.last_kernel_set(), path=m.last_sample_path())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
