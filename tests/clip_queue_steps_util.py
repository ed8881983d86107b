"""Shared by tests/test_emu_clip_queue_steps.py (CPU, the SIMT emulator) and tests/test_gpu_clip_queue_steps.py (MI355X): the checks of
per-clip skip_timesteps in the clip queue (dsg_sample_clip_queue_steps / dsg_clip_queue_plan_steps; the "skip_timesteps" key of
`DSGDiffusion.sample_clip_queue` and `sample.generate_clip_queue[_dsgplus]`), written once over a `DSGLibrary`.  Every comparison is
`np.array_equal`: a clip out of the queue against the same clip sampled alone on a batch-1 handle through the existing clip drivers
(`windows="library"`, `skip_timesteps=` the clip's own) with the same kernel set named on both sides.  All loops are at most six steps."""
import ctypes

import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.model import ClassifierFreeSampleModel
from diffusestylegesture_amd.synth import synth_window_inputs
from tests import clip_queue_edit_util as E
from tests.clip_inpaint_util import n_out_of
from tests.clip_queue_edit_util import ASSIGN_A, ASSIGN_B, BOTH, INIT, INP, NONE, _b1, diffusion_4, edits_of
from tests.clip_queue_util import PAIRS, PLANS, SHARED, SKIP, _after, accepted_sets, clips_of, diffusion, model, queue_jobs, y_of      # noqa: F401

N_SCHED = 1000
KS_MAIN = PLANS[0][0]                    # (1, 3, 2, 1, 2) over 2 slots
SKIPS_MAIN = (996, 994, 999, 998, 996)   # n_run 4, 6, 1, 2, 4; the keyword stays SKIP = 996, so jobs 0 and 4 run at the call's skip
# With the plan of dsg_clip_queue_plan_steps (deepest first) slot 0 runs job 1 (rounds 0-2) and job 3, slot 1 runs job 4 (rounds 0-1), job 0 and
# job 2 (rounds 3-4: its last round beside a dead slot): rounds of 6, 6, 6, 2 and 1 steps, holds 0 / 2 (a slot's first window and later ones), 0 / 1
# and 0; job 2 runs the single last step.  The deeper holds 3 and 5 are in KS_DEEP / SKIPS_DEEP, one round of three slots and one of two
KS_DEEP, SKIPS_DEEP, KINDS_DEEP = (2, 2, 1), (994, 999, 997), (INIT, BOTH, NONE)
CROSS = ((False, True, ASSIGN_B), (True, False, ASSIGN_A))


# ---- the plan, restated -------------------------------------------------------------------------------------------------------------------
def plan_py(K, n_slots, n_run=None):
    """the rule of dsg_clip_queue_plan_steps: jobs by n_run descending, K descending, index ascending; each to the slot with the fewest
    rounds so far (ties: lowest slot); total_steps = the sum over the rounds of the largest n_run alive (n_run None: n_rounds)"""
    n = len(K)
    order = sorted(range(n), key=lambda j: (-(n_run[j] if n_run is not None else 0), -K[j], j))
    load, slot, first = [0] * n_slots, [0] * n, [0] * n
    for j in order:
        s = min(range(n_slots), key=lambda t: (load[t], t))
        slot[j], first[j] = s, load[s]
        load[s] += K[j]
    n_rounds = max(load)
    if n_run is None:
        return slot, first, n_rounds, n_rounds
    total = sum(max(n_run[j] for j in range(n) if first[j] <= r < first[j] + K[j]) for r in range(n_rounds))
    return slot, first, n_rounds, total


def plan_raw(lib, K, n_slots, n_run=None, want_total=True):
    k = np.ascontiguousarray(K, np.int32)
    nr = None if n_run is None else np.ascontiguousarray(n_run, np.int32)
    slot, first, n_rounds, total = np.zeros(len(k), np.int32), np.zeros(len(k), np.int32), ctypes.c_int32(0), ctypes.c_int64(-1)
    rc = lib.cdll.dsg_clip_queue_plan_steps(k.ctypes.data, None if nr is None else nr.ctypes.data, len(k), n_slots, slot.ctypes.data,
                                            first.ctypes.data, ctypes.byref(n_rounds), ctypes.byref(total) if want_total else None)
    assert rc == 0, lib.cdll.dsg_last_error()
    return slot.tolist(), first.tolist(), int(n_rounds.value), int(total.value)


MIXED_PLANS = (                                        # K, n_run, slots
    (KS_MAIN, (4, 6, 1, 2, 4), 2),                     # check 1: ties in n_run broken by K
    ((2, 2, 1, 2, 1, 3), (5, 5, 5, 2, 2, 2), 2),       # ties in n_run AND K: index order
    ((2, 1, 3, 1, 1, 2), (4, 6, 2, 1, 5, 3), 4),       # check 4: six different depths
    ((1, 1, 1, 1, 1, 1, 1), (3, 1, 3, 1, 3, 1, 3), 3),
    ((3, 3), (1, 1000), 5),                            # more slots than jobs
)


def check_plan(lib):
    for K, n_slots, slot, first, n_rounds in PLANS:
        assert plan_raw(lib, K, n_slots) == (list(slot), list(first), n_rounds, n_rounds), (K, n_slots)
        assert plan_py(K, n_slots) == (list(slot), list(first), n_rounds, n_rounds), (K, n_slots)
        assert L.clip_queue_plan(K, n_slots, lib) == (list(slot), list(first), n_rounds)
        # all n_run equal: the same plan, every round that long
        assert plan_raw(lib, K, n_slots, [7] * len(K)) == (list(slot), list(first), n_rounds, 7 * n_rounds)
    for K, n_run, n_slots in MIXED_PLANS:
        want = plan_py(K, n_slots, n_run)
        assert plan_raw(lib, K, n_slots, n_run) == want, (K, n_run, n_slots)
        assert L.clip_queue_plan(K, n_slots, lib, n_run=n_run) == want
        assert plan_raw(lib, K, n_slots, n_run, want_total=False)[:3] == want[:3]      # total_steps is nullable
    assert plan_py(*MIXED_PLANS[0][::2], MIXED_PLANS[0][1])[3] == 21
    # the worked example of include/dsg.h: 24 fresh clips and 24 edits of 100 steps, K = 4, 16 slots
    for K, n_run in (([4] * 48, [1000] * 24 + [100] * 24), ([4] * 48, [1000, 100] * 24)):
        slot, first, n_rounds, total = plan_raw(lib, K, 16, n_run)
        assert (n_rounds, total) == (12, 8400)
    assert plan_raw(lib, [4] * 24, 16, [1000] * 24)[3] + plan_raw(lib, [4] * 24, 16, [100] * 24)[3] == 8800
    one, r = np.ones(1, np.int32), ctypes.c_int32(0)
    for K, nr, n_jobs, n_slots in (([0], [1], 1, 1), ([1], [0], 1, 1), ([1], [1], 0, 1), ([1], [1], 1, 0)):
        k, n = np.array(K, np.int32), np.array(nr, np.int32)
        assert lib.cdll.dsg_clip_queue_plan_steps(k.ctypes.data, n.ctypes.data, n_jobs, n_slots, one.ctypes.data, one.ctypes.data,
                                                  ctypes.byref(r), None) == L.E_INVALID


# ---- the queue ------------------------------------------------------------------------------------------------------------------------------
def queue(cfg, lanes, d, clips, pairs, edits, skips, B, ddim=False, root_shift=True, skip=SKIP):
    """skips: one per clip (None: the clip carries no key and takes the keyword's)"""
    d.manual_seed(SHARED, 99)
    jobs = [dict(j, **e, **({} if s is None else {"skip_timesteps": s})) for j, e, s in zip(queue_jobs(cfg, clips, pairs), edits, skips)]
    return d.sample_clip_queue(lanes, jobs, B, root_shift=root_shift, keep_last_tail=False, ddim=ddim, eta=0.5, skip_timesteps=skip)


def _steps_of(d, Ks, skips, n_slots):
    return plan_py(Ks, n_slots, [d.num_timesteps - s for s in skips])[3]


# ---- 1. mixed strengths ------------------------------------------------------------------------------------------------------------------
def check_mixed(lib, cfg, prec, kset, cases=((False, True, ASSIGN_A), (True, False, ASSIGN_B)), Ks=KS_MAIN, skips=SKIPS_MAIN, B=2, skip=SKIP,
                make_diffusion=diffusion):
    """cases: (ddim, root_shift, job -> edits).  Every job equals the clip alone at ITS skip; every job whose skip differs from the keyword's
    differs from the same queue run with the keyword's skip for all (a hold ignored in both runs would otherwise pass against nothing);
    n_steps of the timing report is the plan's total"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), make_diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    for ddim, root_shift, kinds in cases:
        kw = dict(ddim=ddim, root_shift=root_shift, skip=skip)
        edits = edits_of(cfg, Ks, False, kinds)
        flat = E.queue(cfg, mB, d, clips, pairs, edits, B, **kw)
        draw0 = d._draw
        got = queue(cfg, mB, d, clips, pairs, edits, [None if s == skip else s for s in skips], B, **kw)
        assert mB.last_kernel_set() == kset and mB.noise_streams is None and not mB.inpainting
        assert mB.last_sample_ms()[1] == _steps_of(d, Ks, skips, B), (mB.last_sample_ms(), _steps_of(d, Ks, skips, B))
        assert d._draw == max(K * (1 + d.num_timesteps - s) for K, s in zip(Ks, skips)) and draw0 == max(Ks) * (1 + d.num_timesteps - skip)
        for i, (clip, pair) in enumerate(zip(clips, pairs)):
            want = E.alone(cfg, m1, d, clip, pair, edits[i], ddim=ddim, root_shift=root_shift, skip=skips[i])
            assert m1.last_kernel_set() == kset
            assert got[i].shape == want.shape == (n_out_of(cfg, Ks[i], False), cfg.njoints)
            assert np.array_equal(got[i], want), (cfg.name, prec, kset, ddim, root_shift, kinds, i, float(np.max(np.abs(got[i] - want))))
            assert np.array_equal(got[i], flat[i]) == (skips[i] == skip), (cfg.name, prec, kset, ddim, root_shift, kinds, i)


def check_deep_holds(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """holds of 5 and 3 beside a job that runs all six steps, in a slot's first window and in its second; DDIM with eta = 0 too -- no step
    draws noise there, the hold must still hold"""
    check_mixed(lib, cfg, prec, kset, cases=((False, True, KINDS_DEEP),), Ks=KS_DEEP, skips=SKIPS_DEEP, B=3)
    mB, m1, d = model(lib, cfg, prec, 3, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, KS_DEEP), PAIRS[:3]
    d.manual_seed(SHARED, 99)
    jobs = [dict(j, skip_timesteps=s) for j, s in zip(queue_jobs(cfg, clips, pairs), SKIPS_DEEP)]
    got = d.sample_clip_queue(mB, jobs, 3, root_shift=True, keep_last_tail=False, ddim=True, eta=0.0, skip_timesteps=SKIP)
    for i, (clip, (seed, sid)) in enumerate(zip(clips, pairs)):
        want = S.generate_clip(m1, d, list(clip["feats"]), clip["style"], seed=seed, smoothing=True, skip_timesteps=SKIPS_DEEP[i], stream_id=sid,
                               seed_pose=clip["seed"], windows="library", ddim=True, eta=0.0)[0]
        assert np.array_equal(got[i], want), i


# ---- 2. fresh beside edits, four-step respaced schedule ------------------------------------------------------------------------------------
def check_fresh_beside_edits(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """skips (0, 2, 3) of four steps, B = 2: job 0 starts from the draw itself and runs all four steps, job 1 from q_sample of its init at
    timestep index 1, job 2 from q_sample of zero at index 0 -- the three start forms and holds 0 / 2 / 3 in one batch"""
    check_mixed(lib, cfg, prec, kset, cases=((False, True, (NONE, INIT, NONE)),), Ks=(2, 1, 1), skips=(0, 2, 3), skip=0,
                make_diffusion=diffusion_4)


# ---- 3. DSG+ stitching; guidance and variant 5 -----------------------------------------------------------------------------------------------
SKIPS_3 = (996, 998, 994)


def check_dsgplus(lib, cfg=C.TINY4, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(NONE, INIT, BOTH), skips=SKIPS_3, B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    edits = edits_of(cfg, Ks, True, kinds)
    real = [K * cfg.stride - 3 * i for i, K in enumerate(Ks)]
    dicts = [dict({"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"], "real_n_frames": r,
                   "clip_id": i}, **e) for c, r, i, e in zip(clips, real, ids, edits)]
    run = lambda ds: S.generate_clip_queue_dsgplus(mB, d, ds, seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=None, B=B)
    flat = run(dicts)
    got = run([dict(c, skip_timesteps=s) for c, s in zip(dicts, skips)])
    assert mB.last_kernel_set() == kset and mB.last_sample_ms()[1] == _steps_of(d, Ks, skips, B)
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        want = E.alone(cfg, m1, d, clip, (SHARED, sid), edits[i], skip=skips[i])[:real[i]]
        assert got[i].shape == (real[i], cfg.njoints) and np.array_equal(got[i], want), (cfg.name, i)
        assert np.array_equal(got[i], flat[i]) == (skips[i] == SKIP), i


def check_guided_v5(lib, cfg=C.TINY5, prec="bf16", kset="tile", Ks=(2, 1, 2), scales=(2.5, 1.0, 0.5), kinds=(BOTH, NONE, INIT), skips=SKIPS_3, B=2,
                    keep_last_tail=True, clips=None):
    """under guidance a held element's unconditional twin must hold too: the twin rows are written by the conditional element's epilogue"""
    mB, m1, d = model(lib, cfg, prec, 2 * B, kset), model(lib, cfg, prec, 2, kset), diffusion(lib)
    clips = clips_of(cfg, Ks) if clips is None else clips
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    edits = edits_of(cfg, Ks, keep_last_tail, kinds)
    dicts = [dict({"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"], "real_n_frames": K * cfg.stride,
                   "clip_id": i, "scale": s}, **e) for c, K, i, s, e in zip(clips, Ks, ids, scales, edits)]
    run = lambda ds: S.generate_clip_queue_dsgplus(ClassifierFreeSampleModel(mB), d, ds, seed=SHARED, skip_timesteps=SKIP, feature_division=1,
                                                   kernel_set=None, B=B)
    flat = run(dicts)
    got = run([dict(c, skip_timesteps=s) for c, s in zip(dicts, skips)])
    assert mB.last_kernel_set() == kset
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        audio = [S._dsgplus_window_y(cfg, list(clip["feats"]), w, None, clip["seed"], clip["seed_last"], False, None)["audio"] for w in range(Ks[i])]
        d.manual_seed(SHARED, sid)
        want = d.sample_clip(ClassifierFreeSampleModel(m1), audio, clip["style"], seed0=clip["seed"], root_shift=False, keep_last_tail=True,
                             skip_timesteps=skips[i], scale=np.array([scales[i]], np.float32), seed_last=clip["seed_last"], **_b1(edits[i]))[0]
        assert m1.last_kernel_set() == kset
        assert np.array_equal(got[i], want), (cfg.name, i, float(np.max(np.abs(got[i] - want))))
        assert np.array_equal(got[i], flat[i]) == (skips[i] == SKIP), i


# ---- 4. lanes -------------------------------------------------------------------------------------------------------------------------------
def check_lanes(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=PLANS[1][0], kinds=(BOTH, NONE, INIT, INP, NONE, INP),
                skips=(996, 994, 998, 999, 995, 997)):
    d = diffusion(lib)
    base = model(lib, cfg, prec, 4, kset)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    per = {}
    for n_lanes, B in ((2, 2), (1, 4), (4, 1)):
        lanes = [base] + [base.clone(B) for _ in range(n_lanes - 1)]
        per[n_lanes] = queue(cfg, lanes, d, clips, pairs, edits, skips, B)
        assert all(ln.last_kernel_set() == kset and ln.noise_streams is None and not ln.inpainting for ln in lanes)
        assert all(ln.last_sample_ms()[1] == _steps_of(d, Ks, skips, 4) for ln in lanes)
    m1 = model(lib, cfg, prec, 1, kset)
    for i in range(len(Ks)):
        assert np.array_equal(per[2][i], per[1][i]) and np.array_equal(per[2][i], per[4][i]), i
        assert np.array_equal(per[2][i], E.alone(cfg, m1, d, clips[i], pairs[i], edits[i], skip=skips[i])), i


# ---- 5. the raw export ----------------------------------------------------------------------------------------------------------------------
def _raw(lib, handles, cfg, clips, pairs, edits, skips, B, device=False, args_skip=SKIP):
    """dsg_sample_clip_queue_steps through ctypes alone: (return code, message, [out per clip, two guard rows behind it]).  edits: None (a
    NULL array) or one dict per clip; skips: None (NULL) or one int per clip; device: every edit tensor and `out` as torch device tensors"""
    jobs, eds = (L.dsg_clip_job * len(clips))(), (L.dsg_clip_edit * len(clips))()
    keep, outs = [], []
    if device:
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        ptr = lambda t: t.data_ptr()
    else:
        dev = np.ascontiguousarray
        ptr = lambda a: a.ctypes.data
    for j, (job, ed, c, (seed, sid)) in enumerate(zip(jobs, eds, clips, pairs)):
        K = len(c["feats"])
        audio = np.ascontiguousarray(np.concatenate(c["feats"]), np.float32)
        out = dev(np.full((n_out_of(cfg, K, False) + 2, cfg.njoints), 7.0, np.float32))
        keep += [audio, out]
        outs.append(out)
        job.style, job.seed0, job.audio, job.out = c["style"].ctypes.data, c["seed"].ctypes.data, audio.ctypes.data, ptr(out)
        job.K, job.scale, job.seed, job.stream_id = K, 1.0, seed, sid
        for key, field in (("inpainting_mask", "inp_mask"), ("inpainted_motion", "inp_motion"), ("init_motion", "init_motion")):
            if edits is not None and key in edits[j]:
                t = dev(edits[j][key])
                keep.append(t)
                setattr(ed, field, ptr(t))
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps = L.MODE_DDPM, args_skip
    hs = (ctypes.c_void_p * len(handles))(*handles)
    sk = None if skips is None else np.asarray(skips, np.int32)
    ones = np.ones(cfg.n_poses, np.uint8)
    rc = lib.cdll.dsg_sample_clip_queue_steps(hs, len(handles), jobs, None if edits is None else eds, None if sk is None else sk.ctypes.data,
                                              len(clips), B, ones.ctypes.data, 0, ctypes.byref(a), 1, 0, L.current_stream_ptr() if device else None)
    if device:
        import torch
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in outs]
    return rc, (lib.cdll.dsg_last_error() or b"").decode(), outs


def check_raw_and_state(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(BOTH, INP, INIT), skips=SKIPS_3, B=2):
    d = diffusion(lib)
    shape = (2, cfg.njoints, 1, cfg.n_poses)
    y = y_of(cfg, (10, 11))
    one_step = lambda m: np.asarray(d.manual_seed(SHARED, 3).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y},
                                                                            skip_timesteps=d.num_timesteps - 1))
    fresh_after = _after(lib, cfg, model(lib, cfg, prec, 2, kset), d)
    fresh_step = one_step(model(lib, cfg, prec, 2, kset))
    m = model(lib, cfg, prec, B, kset)
    m.set_schedule(d)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    # skip_timesteps == NULL, an array of -1 and an array of the call's skip are dsg_sample_clip_queue_edit, with and without edits
    for e in (None, edits):
        rc, msg, old = E._raw(lib, [m.handle], cfg, clips, pairs, e, B)
        assert rc == 0, msg
        for sk in (None, [-1] * len(Ks), [SKIP] * len(Ks), [-1, SKIP, -1]):
            rc, msg, new = _raw(lib, [m.handle], cfg, clips, pairs, e, sk, B)
            assert rc == 0, msg
            assert all(np.array_equal(a, b) for a, b in zip(old, new)), sk
            assert m.last_sample_ms()[1] == L.clip_queue_plan(Ks, B, lib)[2] * (N_SCHED - SKIP)
    # the raw call with host pointers is what the Python layer returns
    rc, msg, got = _raw(lib, [m.handle], cfg, clips, pairs, edits, skips, B)
    assert rc == 0, msg
    want = queue(cfg, m, d, clips, pairs, edits, skips, B)
    for i in range(len(Ks)):
        assert np.array_equal(got[i][:-2], want[i]) and (got[i][-2:] == 7.0).all(), i
        assert np.array_equal(got[i], old[i]) == (skips[i] == SKIP), i
    # an entry < 0 is the call's skip: the same bits with the call's skip moved
    rc, msg, sub = _raw(lib, [m.handle], cfg, clips, pairs, edits, [-1, skips[1], skips[2]], B, args_skip=skips[0])
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, sub)), msg
    # after such a call the handle samples what a fresh handle samples
    assert not m.inpainting and m.noise_streams is None
    used = _after(lib, cfg, m, d)
    assert len(used) == len(fresh_after) and all(np.array_equal(a, b) for a, b in zip(fresh_after, used))
    # a skip of n, and a skip of -5 after the substitution, are refused with the job's number; the handle is as it came
    for sk, args_skip, job in (([996, N_SCHED, 996], SKIP, 1), ([996, 994, -1], -5, 2), (None, -5, 0), ([996, 994, N_SCHED + 7], SKIP, 2)):
        rc, msg, _ = _raw(lib, [m.handle], cfg, clips, pairs, edits, sk, B, args_skip=args_skip)
        assert rc == L.E_INVALID and f"job {job}" in msg and "skip_timesteps" in msg, (rc, msg)
        assert np.array_equal(one_step(m), fresh_step), sk
    # everything dsg_sample_clip_queue_edit refuses
    n_out = n_out_of(cfg, 2, False)
    m.set_clip_init(np.zeros((2, n_out, cfg.njoints), np.float32), 2)
    rc, msg, _ = _raw(lib, [m.handle], cfg, clips, pairs, edits, skips, B)
    assert rc == L.E_INVALID and "clip-level init motion" in msg, (rc, msg)
    m.set_clip_init(None, 0)
    half = [dict(e) for e in edits]
    del half[1]["inpainted_motion"]
    rc, msg, _ = _raw(lib, [m.handle], cfg, clips, pairs, half, skips, B)
    assert rc == L.E_INVALID and "go together" in msg and "job 1" in msg, (rc, msg)
    assert np.array_equal(one_step(m), fresh_step)
    # the Python layer validates with the clip's number
    import pytest
    jobs = queue_jobs(cfg, clips, pairs)
    kw = dict(root_shift=True, keep_last_tail=False, skip_timesteps=SKIP)
    for bad in (N_SCHED, -1):
        with pytest.raises(ValueError, match="clip 2.*skip_timesteps"):
            d.sample_clip_queue(m, [jobs[0], jobs[1], dict(jobs[2], skip_timesteps=bad)], B, **kw)
    with pytest.raises(ValueError, match="n_run has 2 entries"):
        L.clip_queue_plan(Ks, B, lib, n_run=[1, 2])
    assert np.array_equal(one_step(m), fresh_step)


def check_device_pointers(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(INP, INIT, BOTH), skips=SKIPS_3, B=2):
    m, d = model(lib, cfg, prec, B, kset), diffusion(lib)
    m.set_schedule(d)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    want = queue(cfg, m, d, clips, pairs, edits, skips, B)
    rc, msg, got = _raw(lib, [m.handle], cfg, clips, pairs, edits, skips, B, device=True)
    assert rc == 0, msg
    for i in range(len(Ks)):
        assert np.array_equal(got[i][:-2], want[i]) and (got[i][-2:] == 7.0).all(), i


def check_abi(lib):
    E.check_abi(lib)
    assert ctypes.sizeof(L.dsg_clip_job) == 80
    for name in ("dsg_sample_clip_queue_steps", "dsg_clip_queue_plan_steps"):
        assert name in L.SYMBOLS and hasattr(lib.cdll, name)


# ---- 7. product widths (GPU only) ------------------------------------------------------------------------------------------------------------
def check_zeggs_rows(lib):
    """the streaming pose head k_ws<EPI_OUT> of the ROWS set at the ZEGGS widths"""
    cfg, Ks, B, kinds, skips = C.ZEGGS, PLANS[2][0], 3, (BOTH, NONE, NONE, NONE), (996, 998, 994, 999)
    mB, m1, d = model(lib, cfg, "bf16", B, "rows"), model(lib, cfg, "bf16", 1, "rows"), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:4]
    edits = edits_of(cfg, Ks, False, kinds)
    flat = E.queue(cfg, mB, d, clips, pairs, edits, B)
    got = queue(cfg, mB, d, clips, pairs, edits, skips, B)
    assert mB.last_kernel_set() == "rows" and mB.last_sample_ms()[1] == _steps_of(d, Ks, skips, B)
    for i in range(4):
        want = E.alone(cfg, m1, d, clips[i], pairs[i], edits[i], skip=skips[i])
        assert m1.last_kernel_set() == "rows"
        assert np.array_equal(got[i], want), (i, float(np.max(np.abs(got[i] - want))))
        assert np.array_equal(got[i], flat[i]) == (skips[i] == SKIP), i


def check_beat_rows_guided(lib):
    """the guided streaming pose head k_ws_cfg of the ROWS set at the BEAT width: two K = 1 jobs, B = 2 plus twins, skips (998, 996)"""
    cfg = C.BEATPP
    clips = []
    for cid in (20, 21):      # as clip_queue_util.clip_of, with the stride-long windows of the DSG+ config of the same widths
        y0 = synth_window_inputs(cfg, 1, window=0, clips=[cid], seed_pose_scale=0.3)
        style = np.zeros((1, cfg.style_dim_in), np.float32)
        style[0, cid % cfg.style_dim_in] = 1.0
        clips.append({"feats": (synth_window_inputs(C.BEAT, 1, window=0, clips=[cid])["audio"],), "style": style, "seed": y0["seed"],
                      "seed_last": y0["seed_last"]})
    check_guided_v5(lib, cfg, "bf16", "rows", Ks=(1, 1), scales=(2.5, 0.5), kinds=(NONE, NONE), skips=(998, 996), B=2, clips=clips)
