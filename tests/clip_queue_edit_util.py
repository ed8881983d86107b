"""Shared by tests/test_emu_clip_queue_edit.py (CPU, the SIMT emulator) and tests/test_gpu_clip_queue_edit.py (MI355X): the checks of per-clip
edits in the clip queue (dsg_sample_clip_queue_edit; the "inpainting_mask" / "inpainted_motion" / "init_motion" keys of
`DSGDiffusion.sample_clip_queue` and `sample.generate_clip_queue[_dsgplus]`), written once over a `DSGLibrary`.  Every comparison is
`np.array_equal`: a clip out of the queue against the same clip sampled alone on a batch-1 handle through the existing clip drivers
(`windows="library"`: dsg_set_clip_inpainting / dsg_set_clip_init + dsg_sample_clip) with the same kernel set named on both sides.  All loops
are four steps."""
import ctypes

import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
from diffusestylegesture_amd.model import ClassifierFreeSampleModel
from tests.clip_init_util import clip_init
from tests.clip_inpaint_util import n_out_of
from tests.clip_queue_util import (PAIRS, PLANS, SHARED, SKIP, _after, _zeggs_like, accepted_sets, clips_of, diffusion, model,      # noqa: F401
                                   queue_jobs, y_of)

NONE, INP, INIT, BOTH = 0, 1, 2, 3
KS_MAIN = PLANS[0][0]                  # (1, 3, 2, 1, 2) over 2 slots: slot 0 runs job 1, 0, 3; slot 1 runs job 2, 4, then is dead
# job -> edits.  A: slot 0 is refilled from an edited clip (1) to a plain one (0) and on to a constrained K = 1 clip (3), beside an init-only
# neighbour (2) on another window index and, in the last round, a dead slot.  B: slot 0 goes plain (1) -> init-only K = 1 (0) -> both (3);
# slot 1 plain (2) -> constrained (4) -> dead.  The K = 1 jobs hold the seed frames df < 0 and the held closing pose df >= n_out in one window
ASSIGN_A = (NONE, BOTH, INIT, INP, NONE)
ASSIGN_B = (INIT, NONE, NONE, BOTH, INP)
CROSS = ((False, True, ASSIGN_B), (True, False, ASSIGN_A))      # the other pairing of assignment and sampler, run under TILE


def diffusion_4(lib):
    """a respaced schedule of four steps (timesteps 0, 333, 666, 999), for skip_timesteps = 0: as clip_queue_util.diffusion_respaced"""
    return create_gaussian_diffusion("4", library=lib)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def edit_of(cfg, K, keep_last_tail, cid, kind):
    """the edits of clip `cid` as the dict keys of the queue, each [n_out, J].  Constraint: every third feature (3, 6, ...; two of the set
    bytes are not 1) on a band of frames around the first hand-off -- rows keep - S - 3 .. keep + 2, which window 0 writes, window 0's tail
    carries and window 1 blends -- clipped to the clip, plus the three root channels on row 2; motion 0.5 * randn.  Init: clip_init with the
    clip's own seed."""
    n_out, J, keep, Sd = n_out_of(cfg, K, keep_last_tail), cfg.njoints, cfg.stride, cfg.n_seed
    e = {}
    if kind & INP:
        mask = np.zeros((n_out, J), np.uint8)
        lo, hi = keep - Sd - 3, min(n_out, keep + 3)
        assert 2 < lo < hi
        mask[lo:hi, 3::3] = 1
        mask[lo, 3], mask[hi - 1, 6] = 255, 2
        mask[2, :3] = 1
        e["inpainting_mask"] = mask
        e["inpainted_motion"] = (0.5 * np.random.default_rng(100 + cid).standard_normal((n_out, J))).astype(np.float32)
    if kind & INIT:
        e["init_motion"] = clip_init(cfg, 1, K, keep_last_tail, seed=200 + cid)[0]
    return e


def edits_of(cfg, Ks, keep_last_tail, kinds):
    return [edit_of(cfg, K, keep_last_tail, i, kind) for i, (K, kind) in enumerate(zip(Ks, kinds))]


def _b1(edit):
    """the edits as the batch-1 drivers take them: [1, n_out, J]"""
    return {k: v[None] for k, v in edit.items()}


# ---- the clip alone, and the queue ---------------------------------------------------------------------------------------------------------
def alone(cfg, m1, d, clip, pair, edit, ddim=False, root_shift=True, skip=SKIP):
    """the clip with its edits on a batch-1 handle through the existing driver (dsg_set_clip_* + dsg_sample_clip): [n_out, J]"""
    seed, sid = pair
    if _zeggs_like(cfg):
        return S.generate_clip(m1, d, list(clip["feats"]), clip["style"], seed=seed, smoothing=root_shift, skip_timesteps=skip, stream_id=sid,
                               seed_pose=clip["seed"], windows="library", ddim=ddim, eta=0.5, **_b1(edit))[0]
    K = len(clip["feats"])
    return S.generate_clip_dsgplus(m1, d, list(clip["feats"]), clip["style"], clip["seed"], K * cfg.stride, seed=seed, skip_timesteps=skip,
                                   stream_id=sid, seed_last=clip["seed_last"], feature_division=1, windows="library", ddim=ddim, eta=0.5,
                                   **_b1(edit))[0]


def queue(cfg, lanes, d, clips, pairs, edits, B, ddim=False, root_shift=True, skip=SKIP):
    d.manual_seed(SHARED, 99)
    jobs = [dict(j, **e) for j, e in zip(queue_jobs(cfg, clips, pairs), edits)]
    return d.sample_clip_queue(lanes, jobs, B, root_shift=root_shift, keep_last_tail=False, ddim=ddim, eta=0.5, skip_timesteps=skip)


# ---- 1. the mixed queue -------------------------------------------------------------------------------------------------------------------
def check_mixed(lib, cfg, prec, kset, cases=((False, True, ASSIGN_A), (True, False, ASSIGN_B)), Ks=KS_MAIN, B=2, skip=SKIP,
                make_diffusion=diffusion):
    """cases: (ddim, root_shift, job -> edits).  Every job of the queue equals the clip alone with its edits; every edited job differs from the
    same job unedited (a cut kernel that wrote "unmasked" everywhere, or a start kernel that ignored the init, would otherwise pass against
    nothing)"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), make_diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    no_edits = [{}] * len(Ks)
    plains = {}
    for ddim, root_shift, kinds in cases:
        kw = dict(ddim=ddim, root_shift=root_shift, skip=skip)
        if (ddim, root_shift) not in plains:
            plains[ddim, root_shift] = queue(cfg, mB, d, clips, pairs, no_edits, B, **kw)
        plain = plains[ddim, root_shift]
        edits = edits_of(cfg, Ks, False, kinds)
        got = queue(cfg, mB, d, clips, pairs, edits, B, **kw)
        assert mB.last_kernel_set() == kset and mB.noise_streams is None and not mB.inpainting
        for i, (clip, pair) in enumerate(zip(clips, pairs)):
            want = alone(cfg, m1, d, clip, pair, edits[i], **kw)
            assert m1.last_kernel_set() == kset
            assert got[i].shape == want.shape == (n_out_of(cfg, Ks[i], False), cfg.njoints)
            assert np.array_equal(got[i], want), (cfg.name, prec, kset, ddim, root_shift, kinds, i, float(np.max(np.abs(got[i] - want))))
            assert np.array_equal(got[i], plain[i]) == (kinds[i] == NONE), (cfg.name, prec, kset, ddim, root_shift, kinds, i)
            if kinds[i] & INP:          # the constraint holds where the clip's own frame is written unshifted: window 0's rows
                mk = edits[i]["inpainting_mask"][:cfg.stride - cfg.n_seed] != 0
                assert np.array_equal(got[i][:cfg.stride - cfg.n_seed][mk], edits[i]["inpainted_motion"][:cfg.stride - cfg.n_seed][mk])


def check_skip0(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """skip_timesteps = 0 on a four-step schedule: a job with an init starts from q_sample at the last timestep, its neighbour without one
    from the draw itself -- the two start forms that differ most, in one batch"""
    check_mixed(lib, cfg, prec, kset, cases=((False, True, (INIT, NONE, BOTH)),), Ks=(2, 1, 1), skip=0, make_diffusion=diffusion_4)


# ---- 2. DSG+ stitching ------------------------------------------------------------------------------------------------------------------
def check_dsgplus(lib, cfg=C.TINY4, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(NONE, INIT, BOTH), B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    edits = edits_of(cfg, Ks, True, kinds)
    real = [K * cfg.stride - 3 * i for i, K in enumerate(Ks)]            # every clip its own real_n_frames
    dicts = [{"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"], "real_n_frames": r, "clip_id": i}
             for c, r, i in zip(clips, real, ids)]
    run = lambda ds: S.generate_clip_queue_dsgplus(mB, d, ds, seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=None, B=B)
    plain = run(dicts)
    got = run([dict(c, **e) for c, e in zip(dicts, edits)])
    assert mB.last_kernel_set() == kset
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        want = alone(cfg, m1, d, clip, (SHARED, sid), edits[i])[:real[i]]
        assert got[i].shape == (real[i], cfg.njoints) and np.array_equal(got[i], want), (cfg.name, i)
        assert np.array_equal(got[i], plain[i]) == (kinds[i] == NONE), i


# ---- 3. guidance and variant 5 ------------------------------------------------------------------------------------------------------------
def check_guided_v5(lib, cfg=C.TINY5, prec="bf16", kset="tile", Ks=(2, 1, 2), scales=(2.5, 1.0, 0.5), kinds=(BOTH, NONE, INIT), B=2):
    mB, m1, d = model(lib, cfg, prec, 2 * B, kset), model(lib, cfg, prec, 2, kset), diffusion(lib)
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    edits = edits_of(cfg, Ks, True, kinds)
    dicts = [{"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"], "real_n_frames": K * cfg.stride,
              "clip_id": i, "scale": s} for c, K, i, s in zip(clips, Ks, ids, scales)]
    run = lambda ds: S.generate_clip_queue_dsgplus(ClassifierFreeSampleModel(mB), d, ds, seed=SHARED, skip_timesteps=SKIP, feature_division=1,
                                                   kernel_set=None)
    plain = run(dicts)
    got = run([dict(c, **e) for c, e in zip(dicts, edits)])
    assert mB.last_kernel_set() == kset
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        audio = [S._dsgplus_window_y(cfg, list(clip["feats"]), w, None, clip["seed"], clip["seed_last"], False, None)["audio"] for w in range(Ks[i])]
        d.manual_seed(SHARED, sid)
        want = d.sample_clip(ClassifierFreeSampleModel(m1), audio, clip["style"], seed0=clip["seed"], root_shift=False, keep_last_tail=True,
                             skip_timesteps=SKIP, scale=np.array([scales[i]], np.float32), seed_last=clip["seed_last"], **_b1(edits[i]))[0]
        assert m1.last_kernel_set() == kset
        assert np.array_equal(got[i], want), (cfg.name, i, float(np.max(np.abs(got[i] - want))))
        assert np.array_equal(got[i], plain[i]) == (kinds[i] == NONE), i


# ---- 4. lanes ---------------------------------------------------------------------------------------------------------------------------
def check_lanes(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=PLANS[1][0], kinds=(BOTH, NONE, INIT, INP, NONE, INP)):
    d = diffusion(lib)
    base = model(lib, cfg, prec, 4, kset)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    per = {}
    for n_lanes, B in ((2, 2), (1, 4), (4, 1)):
        lanes = [base] + [base.clone(B) for _ in range(n_lanes - 1)]      # (clones inherit the kernel set)
        per[n_lanes] = queue(cfg, lanes, d, clips, pairs, edits, B)
        assert all(ln.last_kernel_set() == kset and ln.noise_streams is None and not ln.inpainting for ln in lanes)
    m1 = model(lib, cfg, prec, 1, kset)
    for i in range(len(Ks)):
        assert np.array_equal(per[2][i], per[1][i]) and np.array_equal(per[2][i], per[4][i]), i
        assert np.array_equal(per[2][i], alone(cfg, m1, d, clips[i], pairs[i], edits[i])), i


# ---- 5. the raw export: device pointers, edits == NULL, errors, nothing sticks ---------------------------------------------------------------
def _raw(lib, handles, cfg, clips, pairs, edits, B, fn="dsg_sample_clip_queue_edit", device=False, half=None):
    """the export through ctypes alone: (return code, message, [out per clip]).  edits: None (a NULL array) or one dict per clip;
    device: every edit tensor and `out` as torch device tensors; half: (job, key) -- that pointer of that job is nulled"""
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
        rows = n_out_of(cfg, K, False)
        out = dev(np.full((rows + 2, cfg.njoints), 7.0, np.float32))      # two guard rows behind the clip
        keep += [audio, out]
        outs.append(out)
        job.style, job.seed0, job.audio, job.out = c["style"].ctypes.data, c["seed"].ctypes.data, audio.ctypes.data, ptr(out)
        job.K, job.scale, job.seed, job.stream_id = K, 1.0, seed, sid
        for key, field in (("inpainting_mask", "inp_mask"), ("inpainted_motion", "inp_motion"), ("init_motion", "init_motion")):
            if edits is not None and key in edits[j] and half != (j, key):
                t = dev(edits[j][key])
                keep.append(t)
                setattr(ed, field, ptr(t))
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps = L.MODE_DDPM, SKIP
    hs = (ctypes.c_void_p * len(handles))(*handles)
    stream = L.current_stream_ptr() if device else None
    ones = np.ones(cfg.n_poses, np.uint8)                                  # mask_local as `DSGDiffusion.sample_clip_queue` passes it
    tail = (B, ones.ctypes.data, 0, ctypes.byref(a), 1, 0, stream)
    if fn == "dsg_sample_clip_queue":
        rc = lib.cdll.dsg_sample_clip_queue(hs, len(handles), jobs, len(clips), *tail)
    else:
        rc = lib.cdll.dsg_sample_clip_queue_edit(hs, len(handles), jobs, None if edits is None else eds, len(clips), *tail)
    if device:
        import torch
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in outs]
    return rc, (lib.cdll.dsg_last_error() or b"").decode(), outs


def check_device_pointers(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(INP, INIT, BOTH), B=2):
    """the edit tensors and `out` in device memory: read where they are (no staging), the same bits as with host pointers, and nothing is
    written past a clip's last row"""
    m, d = model(lib, cfg, prec, B, kset), diffusion(lib)
    m.set_schedule(d)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    want = queue(cfg, m, d, clips, pairs, edits, B)
    rc, msg, got = _raw(lib, [m.handle], cfg, clips, pairs, edits, B, device=True)
    assert rc == 0, msg
    for i in range(len(Ks)):
        assert np.array_equal(got[i][:-2], want[i]) and (got[i][-2:] == 7.0).all(), i


def check_raw_and_state(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(BOTH, INP, INIT), B=2):
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
    # edits == NULL through the new export is dsg_sample_clip_queue; an array of empty edits too
    rc, msg, old = _raw(lib, [m.handle], cfg, clips, pairs, None, B, fn="dsg_sample_clip_queue")
    assert rc == 0, msg
    for e in (None, [{}] * len(Ks)):
        rc, msg, new = _raw(lib, [m.handle], cfg, clips, pairs, e, B)
        assert rc == 0, msg
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
    # the raw call with host pointers is what the Python layer returns
    rc, msg, got = _raw(lib, [m.handle], cfg, clips, pairs, edits, B)
    assert rc == 0, msg
    want = queue(cfg, m, d, clips, pairs, edits, B)
    for i in range(len(Ks)):
        assert np.array_equal(got[i][:-2], want[i]) and (got[i][-2:] == 7.0).all() and not np.array_equal(got[i], old[i]), i
    # after an edited call the handle samples what a fresh handle samples
    assert not m.inpainting and m.noise_streams is None
    used = _after(lib, cfg, m, d)
    assert len(used) == len(fresh_after) and all(np.array_equal(a, b) for a, b in zip(fresh_after, used))
    # a half-given constraint is refused with the job's number, whichever half is missing; the handle is as it came
    for key in ("inpainting_mask", "inpainted_motion"):
        rc, msg, _ = _raw(lib, [m.handle], cfg, clips, pairs, edits, B, half=(1, key))
        assert rc == L.E_INVALID and "inp_mask and inp_motion go together" in msg and "job 1" in msg, (rc, msg)
        assert np.array_equal(one_step(m), fresh_step), key
    # handles with the sticky setters are still refused, through the new export as through the old one
    n_out = n_out_of(cfg, 2, False)
    for fn in ("dsg_sample_clip_queue", "dsg_sample_clip_queue_edit"):
        e = None if fn == "dsg_sample_clip_queue" else edits
        m.set_clip_inpainting(np.zeros((2, n_out, cfg.njoints), bool), np.zeros((2, n_out, cfg.njoints), np.float32), 2)
        rc, msg, _ = _raw(lib, [m.handle], cfg, clips, pairs, e, B, fn=fn)
        assert rc == L.E_INVALID and "clip-level inpainting" in msg and "dsg_sample_clip_queue_edit" in msg, (rc, msg)
        m.set_clip_inpainting(None, None, 0)
        m.set_clip_init(np.zeros((2, n_out, cfg.njoints), np.float32), 2)
        rc, msg, _ = _raw(lib, [m.handle], cfg, clips, pairs, e, B, fn=fn)
        assert rc == L.E_INVALID and "clip-level init motion" in msg and "dsg_sample_clip_queue_edit" in msg, (rc, msg)
        m.set_clip_init(None, 0)
        assert np.array_equal(one_step(m), fresh_step), fn
    # the Python layer: both or neither, and the shape, with the clip named
    import pytest
    jobs = queue_jobs(cfg, clips, pairs)
    kw = dict(root_shift=True, keep_last_tail=False, skip_timesteps=SKIP)
    with pytest.raises(ValueError, match="clip 1.*go together"):
        d.sample_clip_queue(m, [jobs[0], dict(jobs[1], inpainting_mask=edits[1]["inpainting_mask"]), jobs[2]], B, **kw)
    with pytest.raises(ValueError, match="clip 2.*init_motion shape"):
        d.sample_clip_queue(m, [jobs[0], jobs[1], dict(jobs[2], init_motion=edits[2]["init_motion"][:-1])], B, **kw)
    assert np.array_equal(one_step(m), fresh_step)


# ---- 6. product widths (GPU only) -----------------------------------------------------------------------------------------------------------
def check_zeggs_rows(lib):
    cfg, Ks, B, kinds = C.ZEGGS, PLANS[2][0], 3, (BOTH, NONE, INIT, NONE)
    mB, m1, d = model(lib, cfg, "bf16", B, "rows"), model(lib, cfg, "bf16", 1, "rows"), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:4]
    edits = edits_of(cfg, Ks, False, kinds)
    plain = queue(cfg, mB, d, clips, pairs, [{}] * 4, B)
    got = queue(cfg, mB, d, clips, pairs, edits, B)
    assert mB.last_kernel_set() == "rows"
    for i in range(4):
        want = alone(cfg, m1, d, clips[i], pairs[i], edits[i])
        assert m1.last_kernel_set() == "rows"
        assert np.array_equal(got[i], want), (i, float(np.max(np.abs(got[i] - want))))
        assert np.array_equal(got[i], plain[i]) == (kinds[i] == NONE), i


# ---- 7. ABI -------------------------------------------------------------------------------------------------------------------------------
def check_abi(lib):
    assert ctypes.sizeof(L.dsg_clip_edit) == 32
    assert [f[0] for f in L.dsg_clip_edit._fields_] == ["inp_mask", "inp_motion", "init_motion", "reserved"]
    assert "dsg_sample_clip_queue_edit" in L.SYMBOLS and hasattr(lib.cdll, "dsg_sample_clip_queue_edit")
    assert lib.cdll.dsg_version() == 330
