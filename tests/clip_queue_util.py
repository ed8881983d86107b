"""Shared by tests/test_emu_clip_queue.py (CPU, the SIMT emulator) and tests/test_gpu_clip_queue.py (MI355X): the checks of the clip queue
(dsg_clip_queue_plan / dsg_sample_clip_queue, `DSGDiffusion.sample_clip_queue`, `sample.generate_clip_queue[_dsgplus]`), written once over a
`DSGLibrary`.  Every comparison is `np.array_equal`: a clip out of the queue against the same clip sampled alone on a batch-1 handle
(`generate_clip(..., windows="library", stream_id=...)` after the clip's seed) with the same kernel set named on both sides.  All loops are
four steps (skip_timesteps = 996)."""
import ctypes
import functools

import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.model import ClassifierFreeSampleModel
from diffusestylegesture_amd.synth import synth_window_inputs
from tests.noise_streams_util import accepted_sets, diffusion, model, y_of      # noqa: F401  (re-exported for the two test files)

SKIP = 996                             # 1000 - 4: four steps
SHARED = 5                             # the seed of the drivers, which share one
# per clip: (seed, stream id) -- the seeds differ, one stream id is 0, one uses the high word
PAIRS = ((5, 7), (6, 0), (2 ** 40 + 1, 2 ** 33 + 5), (8, 9), (9, 3), (10, 2 ** 32 + 1))
# the reference values of the issue: K, slots -> slot, first_round, n_rounds
PLANS = (((1, 3, 2, 1, 2), 2, (0, 0, 1, 0, 1), (3, 0, 0, 4, 2), 5),
         ((2, 1, 3, 1, 1, 2), 4, (1, 3, 0, 3, 1, 2), (0, 0, 0, 1, 2, 0), 3),
         ((2, 1, 1, 1), 3, (0, 1, 2, 1), (0, 0, 0, 1), 2),
         ((3,), 2, (0,), (0,), 3))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _zeggs_like(cfg):
    return cfg.variant == C.VARIANT_DSG


@functools.lru_cache(maxsize=None)
def _clip_cached(cfg_name, cid, K):
    cfg = C.CONFIGS[cfg_name]
    fc = cfg if _zeggs_like(cfg) else C.TINY4          # DSG+ / DSG++: stride-long windows, as generate_clip_dsgplus takes them
    feats = tuple(synth_window_inputs(fc, 1, window=w, clips=[cid])["audio"] for w in range(K))
    y0 = synth_window_inputs(cfg, 1, window=0, clips=[cid], seed_pose_scale=0.3)
    style = np.zeros((1, cfg.style_dim_in), np.float32)
    style[0, cid % cfg.style_dim_in] = 1.0             # every clip its own style
    return {"feats": feats, "style": style, "seed": y0["seed"], "seed_last": y0.get("seed_last")}


def clip_of(cfg, cid, K):
    """clip `cid` with K windows: per-window features [1, T_a, A_src], style [1, style_dim_in], seed pose [1, J, 1, S] (and seed_last)"""
    return _clip_cached(cfg.name, int(cid), int(K))


def clips_of(cfg, Ks, first_id=20):
    return [clip_of(cfg, first_id + i, K) for i, K in enumerate(Ks)]


def n_out_of(cfg, K, keep_last_tail):
    return K * cfg.stride - (0 if keep_last_tail else cfg.n_seed)


# ---- the clip alone, and the queue ---------------------------------------------------------------------------------------------------------
def alone(cfg, m1, d, clip, pair, ddim=False, root_shift=True):
    """the clip on a batch-1 handle through the existing driver (dsg_sample_clip): [n_out, J]"""
    seed, sid = pair
    if _zeggs_like(cfg):
        return S.generate_clip(m1, d, list(clip["feats"]), clip["style"], seed=seed, smoothing=root_shift, skip_timesteps=SKIP, stream_id=sid,
                               seed_pose=clip["seed"], windows="library", ddim=ddim, eta=0.5)[0]
    K = len(clip["feats"])
    return S.generate_clip_dsgplus(m1, d, list(clip["feats"]), clip["style"], clip["seed"], K * cfg.stride, seed=seed, skip_timesteps=SKIP,
                                   stream_id=sid, seed_last=clip["seed_last"], feature_division=1, windows="library", ddim=ddim, eta=0.5)[0]


def queue_jobs(cfg, clips, pairs, scales=None):
    """the dicts `DSGDiffusion.sample_clip_queue` takes (the ZEGGS layout: the features as they are)"""
    assert _zeggs_like(cfg)
    return [{"feats": c["feats"], "style": c["style"], "seed0": c["seed"], "stream": p, "scale": None if scales is None else scales[i]}
            for i, (c, p) in enumerate(zip(clips, pairs))]


def queue(cfg, lanes, d, clips, pairs, B, ddim=False, root_shift=True):
    d.manual_seed(SHARED, 99)
    return d.sample_clip_queue(lanes, queue_jobs(cfg, clips, pairs), B, root_shift=root_shift, keep_last_tail=False, ddim=ddim, eta=0.5,
                               skip_timesteps=SKIP)


# ---- 1. the plan (host only) ----------------------------------------------------------------------------------------------------------
def check_plan(lib):
    for K, n_slots, slot, first, n_rounds in PLANS:
        assert L.clip_queue_plan(K, n_slots, lib) == (list(slot), list(first), n_rounds), (K, n_slots)
    rs = np.random.RandomState(0)
    for n_jobs, n_slots in ((48, 16), (7, 3), (3, 8), (1, 1), (20, 1)):
        K = rs.randint(1, 9, size=n_jobs)
        slot, first, n_rounds = L.clip_queue_plan(K, n_slots, lib)
        assert len(slot) == len(first) == n_jobs and all(0 <= s < n_slots for s in slot)            # every job placed once
        busy = np.zeros((n_slots, n_rounds), int)
        for j in range(n_jobs):
            assert first[j] >= 0 and first[j] + K[j] <= n_rounds
            busy[slot[j], first[j]:first[j] + K[j]] += 1
        assert busy.max() == 1                                                                          # no two jobs overlap in a slot
        load = busy.sum(1)
        assert n_rounds == load.max() and load.sum() == K.sum()
        for s in range(n_slots):                                                                        # a slot is filled from round 0 on, no gaps
            assert busy[s, :load[s]].all()
        if n_slots > n_jobs:
            assert (load == 0).sum() == n_slots - n_jobs                                                # empty slots stay empty
    # the workload of tools/clip_queue_bench.py: 269 windows over 16 slots in the lower bound of 17 rounds
    K48 = [4, 2, 5, 16, 1, 2, 8, 2, 4, 12, 1, 8, 3, 1, 2, 5, 5, 2, 3, 2, 8, 5, 1, 12, 2, 3, 16, 16, 12, 1, 12, 12, 5, 1, 3, 1, 8, 2, 3, 5, 2, 8, 2, 12, 3,
           8, 16, 2]
    assert sum(K48) == 269 and L.clip_queue_plan(K48, 16, lib)[2] == 17
    # refusals
    one = np.ones(1, np.int32)
    r = ctypes.c_int32(0)
    for K, n_jobs, n_slots in (([0], 1, 1), ([1], 0, 1), ([1], 1, 0)):
        k = np.array(K, np.int32)
        assert lib.cdll.dsg_clip_queue_plan(k.ctypes.data, n_jobs, n_slots, one.ctypes.data, one.ctypes.data, ctypes.byref(r)) == L.E_INVALID


# ---- 2. each clip equals the clip alone ---------------------------------------------------------------------------------------------------
KS_MAIN = (1, 3, 2, 1, 2)      # over 2 slots: a refill at another window index than the neighbour's, K = 1 (first and last at once), a clip
                               # that starts on the last round, a dead slot in the last round (PLANS[0])


def check_each_clip_alone(lib, cfg, prec, kset, combos=((False, True), (True, False)), Ks=KS_MAIN, B=2):
    """Draw offset at the start kernels: skip_timesteps = 996 > 0 makes k_x_in run q_sample (x = qb z with the init at 0), so the offset of
    the x_T / q_sample draw is covered by every case here -- a slot on window c > 0 that drew window 0's noise would differ from the clip
    alone."""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    for ddim, root_shift in combos:
        got = queue(cfg, mB, d, clips, pairs, B, ddim=ddim, root_shift=root_shift)
        assert mB.last_kernel_set() == kset and mB.noise_streams is None and d._draw == max(Ks) * 5
        assert len(got) == len(Ks)
        for i, (clip, pair) in enumerate(zip(clips, pairs)):
            want = alone(cfg, m1, d, clip, pair, ddim=ddim, root_shift=root_shift)
            assert m1.last_kernel_set() == kset
            assert got[i].shape == want.shape == (n_out_of(cfg, Ks[i], False), cfg.njoints)
            assert np.array_equal(got[i], want), (cfg.name, prec, kset, ddim, root_shift, i, float(np.max(np.abs(got[i] - want))))
        for i in range(len(Ks)):                                           # clips of one length are still different clips
            for k in range(i):
                assert got[i].shape != got[k].shape or not np.array_equal(got[i], got[k]), (i, k)


# ---- 3. DSG+ stitching ------------------------------------------------------------------------------------------------------------------
def check_dsgplus(lib, cfg=C.TINY4, prec="bf16", kset="tile", Ks=(2, 1, 3), B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    real = [K * cfg.stride - 3 * i for i, K in enumerate(Ks)]            # every clip its own real_n_frames
    got = S.generate_clip_queue_dsgplus(mB, d, [{"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"],
                                                 "real_n_frames": r, "clip_id": i} for c, r, i in zip(clips, real, ids)],
                                        seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=None, B=B)
    assert mB.last_kernel_set() == kset
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        want = alone(cfg, m1, d, clip, (SHARED, sid))[:real[i]]
        assert got[i].shape == (real[i], cfg.njoints) and np.array_equal(got[i], want), (cfg.name, i)


# ---- 4. guidance and variant 5 ------------------------------------------------------------------------------------------------------------
def check_guided_v5(lib, cfg=C.TINY5, prec="bf16", kset="tile", Ks=(2, 1, 2), scales=(2.5, 1.0, 0.5), B=2):
    mB, m1, d = model(lib, cfg, prec, 2 * B, kset), model(lib, cfg, prec, 2, kset), diffusion(lib)
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    got = S.generate_clip_queue_dsgplus(ClassifierFreeSampleModel(mB), d,
                                        [{"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"],
                                          "real_n_frames": K * cfg.stride, "clip_id": i, "scale": s}
                                         for c, K, i, s in zip(clips, Ks, ids, scales)],
                                        seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=None)      # B by default: min(4 // 2, 3)
    assert mB.last_kernel_set() == kset
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        audio = [S._dsgplus_window_y(cfg, list(clip["feats"]), w, None, clip["seed"], clip["seed_last"], False, None)["audio"] for w in range(Ks[i])]
        d.manual_seed(SHARED, sid)
        want = d.sample_clip(ClassifierFreeSampleModel(m1), audio, clip["style"], seed0=clip["seed"], root_shift=False, keep_last_tail=True,
                             skip_timesteps=SKIP, scale=np.array([scales[i]], np.float32), seed_last=clip["seed_last"])[0]
        assert m1.last_kernel_set() == kset
        assert np.array_equal(got[i], want), (cfg.name, i, float(np.max(np.abs(got[i] - want))))
    assert not np.array_equal(got[0], got[2])


# ---- 5. lanes ---------------------------------------------------------------------------------------------------------------------------
def check_lanes(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3, 1, 1, 2)):
    d = diffusion(lib)
    base = model(lib, cfg, prec, 4, kset)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    per = {}
    for n_lanes, B in ((2, 2), (1, 4), (4, 1)):
        lanes = [base] + [base.clone(B) for _ in range(n_lanes - 1)]      # (clones inherit the kernel set)
        per[n_lanes] = queue(cfg, lanes, d, clips, pairs, B)
        assert all(ln.last_kernel_set() == kset and ln.noise_streams is None for ln in lanes)
    for i in range(len(Ks)):
        assert np.array_equal(per[2][i], per[1][i]) and np.array_equal(per[2][i], per[4][i]), i
    assert len({g.tobytes() for g in per[2]}) == len(Ks)                   # the six results are pairwise different
    m1 = model(lib, cfg, prec, 1, kset)
    assert np.array_equal(per[2][2], alone(cfg, m1, d, clips[2], pairs[2]))


# ---- 6. more slots than clips, 7. order does not matter ----------------------------------------------------------------------------------
def check_more_slots_and_order(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    mB, m1, d = model(lib, cfg, prec, 2, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clip = clip_of(cfg, 31, 3)
    got = queue(cfg, mB, d, [clip], PAIRS[2:3], 2)                         # slot 1 is dead from round 0
    assert len(got) == 1 and np.array_equal(got[0], alone(cfg, m1, d, clip, PAIRS[2]))
    Ks = (2, 1, 3)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:3]
    fwd = queue(cfg, mB, d, clips, pairs, 2)
    rev = queue(cfg, mB, d, clips[::-1], pairs[::-1], 2)
    for i in range(3):
        assert np.array_equal(fwd[i], rev[2 - i]), i
    # the driver: one seed, clip ids
    ids = [p[1] for p in pairs]
    drv = S.generate_clip_queue(mB, d, [{"feats": c["feats"], "style": c["style"][0], "seed_pose": c["seed"], "clip_id": i} for c, i in zip(clips, ids)],
                                seed=SHARED, skip_timesteps=SKIP, kernel_set=None)
    assert mB.last_kernel_set() == kset
    for i in range(3):
        assert np.array_equal(drv[i], alone(cfg, m1, d, clips[i], (SHARED, ids[i]))), i


# ---- 8. nothing sticks --------------------------------------------------------------------------------------------------------------------
def _after(lib, cfg, m, d):
    """what a handle of batch 2 samples: dsg_sample and dsg_sample_clip, unkeyed and keyed"""
    shape = (2, cfg.njoints, 1, cfg.n_poses)
    y = y_of(cfg, (10, 11))
    clips = clips_of(cfg, (2, 2))
    feats = [np.concatenate([c["feats"][w] for c in clips]) for w in range(2)]
    style, seed = np.concatenate([c["style"] for c in clips]), np.concatenate([c["seed"] for c in clips])
    out = []
    for cs in (None, [7, 2 ** 33 + 5]):
        out.append(np.asarray(d.manual_seed(SHARED, 3).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP,
                                                                      clip_streams=cs)))
        kw = {"stream_id": 3} if cs is None else {"clip_ids": cs}
        out.append(S.generate_clip(m, d, feats, style, seed=SHARED, skip_timesteps=SKIP, seed_pose=seed, windows="library", **kw))
    return out


def check_nothing_sticks(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    d = diffusion(lib)
    fresh = _after(lib, cfg, model(lib, cfg, prec, 2, kset), d)
    m = model(lib, cfg, prec, 2, kset)
    queue(cfg, m, d, clips_of(cfg, KS_MAIN), PAIRS[:5], 2)
    assert m.noise_streams is None
    used = _after(lib, cfg, m, d)
    assert len(fresh) == len(used) == 4 and all(np.array_equal(a, b) for a, b in zip(fresh, used))
    assert m.noise_streams is None


# ---- 9. errors --------------------------------------------------------------------------------------------------------------------------
def _raw(lib, handles, cfg, clips, B, guided=0, edit_args=None, edit_jobs=None, n_jobs=None, keep_last_tail=0):
    """dsg_sample_clip_queue through ctypes alone: (return code, message)"""
    jobs = (L.dsg_clip_job * max(len(clips), 1))()
    keep = []
    for job, c in zip(jobs, clips):
        audio = np.ascontiguousarray(np.concatenate(c["feats"]), np.float32)
        if not _zeggs_like(cfg):
            audio = np.ascontiguousarray(audio[:, :cfg.audio_frames])
        out = np.zeros((n_out_of(cfg, len(c["feats"]), keep_last_tail), cfg.njoints), np.float32)
        keep += [audio, out]
        job.style, job.seed0, job.audio, job.out = c["style"].ctypes.data, c["seed"].ctypes.data, audio.ctypes.data, out.ctypes.data
        job.seed_last = None if c["seed_last"] is None else c["seed_last"].ctypes.data
        job.K, job.scale, job.seed, job.stream_id = len(c["feats"]), 1.0, 5, 7
    if edit_jobs:
        edit_jobs(jobs)
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps = L.MODE_DDPM, SKIP
    if edit_args:
        keep.append(edit_args(a))
    hs = (ctypes.c_void_p * len(handles))(*handles)
    rc = lib.cdll.dsg_sample_clip_queue(hs, len(handles), jobs, len(clips) if n_jobs is None else n_jobs, B, None, guided, ctypes.byref(a), 1,
                                        keep_last_tail, None)
    return rc, (lib.cdll.dsg_last_error() or b"").decode()


def check_errors(lib, cfg=C.TINY, prec="fp32", kset="tile"):
    d = diffusion(lib)
    shape = (2, cfg.njoints, 1, cfg.n_poses)
    y = y_of(cfg, (10, 11))
    one_step = lambda m: np.asarray(d.manual_seed(SHARED, 3).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y},
                                                                            skip_timesteps=d.num_timesteps - 1))
    fresh = one_step(model(lib, cfg, prec, 2, kset))
    m = model(lib, cfg, prec, 2, kset)
    m.set_schedule(d)
    clips = clips_of(cfg, (2, 1))
    buf = np.zeros(shape, np.float32)
    steps = np.zeros(1, np.int32)

    def refused(match, code=L.E_INVALID, handles=None, **kw):
        rc, msg = _raw(lib, [m.handle] if handles is None else handles, cfg, kw.pop("clips", clips), kw.pop("B", 2), **kw)
        assert rc == code and match in msg, (match, rc, msg)
        assert np.array_equal(one_step(m), fresh), match                  # the handle still samples a fresh handle's bits

    refused("n_jobs < 1", n_jobs=0)
    refused("K < 1", edit_jobs=lambda j: setattr(j[1], "K", 0))
    refused("B < 1", B=0)
    refused("exceeds max_batch", B=3)
    refused("max_batch >= 2 * B", B=2, guided=1)
    for name in ("style", "audio", "out"):
        refused("null style / audio / out", edit_jobs=lambda j, name=name: setattr(j[0], name, None))
    for name in ("step_noise", "init_noise", "init_image"):
        refused("not for a queue of clips", edit_args=lambda a, name=name: setattr(a, name, buf.ctypes.data))
    refused("not for a queue of clips", edit_args=lambda a: (setattr(a, "n_dump", 1), setattr(a, "dump_steps", steps.ctypes.data),
                                                             setattr(a, "dump_out", buf.ctypes.data)))
    for name in ("first_step", "max_steps", "const_noise"):
        refused("not for a queue of clips", edit_args=lambda a, name=name: setattr(a, name, 1))
    # lanes: too many, twice the same, another model, another step count
    refused("at most 16 lanes", handles=[m.handle] * 17)
    refused("appears twice", handles=[m.handle, m.handle])
    other = model(lib, C.TINY4, prec, 2, "tile")
    other.set_schedule(d)
    refused("lanes of one model", handles=[m.handle, other.handle])
    lane = m.clone()
    lane.set_schedule(diffusion_respaced(lib))
    refused("one step count", handles=[m.handle, lane.handle])
    # what a handle may not carry
    m.set_noise_streams(None, [1, 2])
    refused("noise streams")
    m.set_noise_streams(None, None)
    mask = np.zeros(shape, bool)
    mask[:, ::3] = True
    m.set_inpainting(mask, buf, 2)
    refused("window-level inpainting")
    m.set_inpainting(None, None, 0)
    n_out = n_out_of(cfg, 2, False)
    m.set_clip_inpainting(np.zeros((2, n_out, cfg.njoints), bool), np.zeros((2, n_out, cfg.njoints), np.float32), 2)
    refused("clip-level inpainting")
    m.set_clip_inpainting(None, None, 0)
    m.set_clip_init(np.zeros((2, n_out, cfg.njoints), np.float32), 2)
    refused("clip-level init motion")
    m.set_clip_init(None, 0)
    # variant 5 without seed_last
    m5 = model(lib, C.TINY5, prec, 2, "tile")
    m5.set_schedule(d)
    rc, msg = _raw(lib, [m5.handle], C.TINY5, clips_of(C.TINY5, (2, 1)), 2, keep_last_tail=1, edit_jobs=lambda j: setattr(j[1], "seed_last", None))
    assert rc == L.E_INVALID and "seed_last" in msg, msg
    # state: before the weights, before the schedule
    from diffusestylegesture_amd.model import DSGDenoiser
    raw = DSGDenoiser(cfg, precision=prec, max_batch=2, library=lib)
    rc, msg = _raw(lib, [raw.handle], cfg, clips, 2)
    assert rc == L.E_STATE and "dsg_finalize_weights" in msg, msg
    loaded = model(lib, cfg, prec, 2, kset)
    rc, msg = _raw(lib, [loaded.handle], cfg, clips, 2)
    assert rc == L.E_STATE and "dsg_set_schedule" in msg, msg
    # and the call itself still works on the handle that was refused so often
    rc, msg = _raw(lib, [m.handle], cfg, clips, 2)
    assert rc == 0, msg
    assert np.array_equal(one_step(m), fresh)


def diffusion_respaced(lib):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    return create_gaussian_diffusion("ddim50", library=lib)


# ---- 10. product widths (GPU only) -----------------------------------------------------------------------------------------------------------
def check_zeggs_rows(lib):
    cfg, Ks, B = C.ZEGGS, (2, 1, 1, 1), 3
    mB, m1, d = model(lib, cfg, "bf16", B, "rows"), model(lib, cfg, "bf16", 1, "rows"), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:4]
    got = queue(cfg, mB, d, clips, pairs, B)
    assert mB.last_kernel_set() == "rows"
    for i in range(4):
        want = alone(cfg, m1, d, clips[i], pairs[i])
        assert m1.last_kernel_set() == "rows"
        assert np.array_equal(got[i], want), (i, float(np.max(np.abs(got[i] - want))))


# ---- 11. every pointer of a job in device memory (GPU only) ----------------------------------------------------------------------------------
def check_device_pointers(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3), B=2):
    """style / seed0 / audio / out as device tensors: the hand-off writes the caller's `out` itself (no staging buffer, no copy at the end);
    the same bits as with host pointers, and nothing is written past a clip's last row"""
    import torch
    m, d = model(lib, cfg, prec, B, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    want = queue(cfg, m, d, clips, pairs, B)
    jobs = (L.dsg_clip_job * len(Ks))()
    keep, outs = [], []
    for job, c, (seed, sid) in zip(jobs, clips, pairs):
        K = len(c["feats"])
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["style"], c["seed"], np.concatenate(c["feats"]))]
        rows = n_out_of(cfg, K, False)
        out = torch.full((rows + 2, cfg.njoints), 7.0, dtype=torch.float32, device="cuda")      # two guard rows behind the clip
        keep += t
        outs.append(out)
        job.style, job.seed0, job.audio, job.out = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr()
        job.K, job.scale, job.seed, job.stream_id = K, 1.0, seed, sid
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps = L.MODE_DDPM, SKIP
    mask = torch.ones(cfg.n_poses, dtype=torch.uint8, device="cuda")
    hs = (ctypes.c_void_p * 1)(m.handle)
    lib.check(lib.cdll.dsg_sample_clip_queue(hs, 1, jobs, len(Ks), B, ctypes.c_void_p(mask.data_ptr()), 0, ctypes.byref(a), 1, 0,
                                             L.current_stream_ptr()))
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        got = out.cpu().numpy()
        assert np.array_equal(got[:-2], want[i]) and (got[-2:] == 7.0).all(), i
