"""Shared by tests/test_emu_noise_streams.py (CPU, the SIMT emulator) and tests/test_gpu_noise_streams.py (MI355X): the checks of per-element
noise streams (dsg_set_noise_streams / dsg_noise_streams, `clip_streams=` of the loops, `clip_ids=` of the clip drivers), written once over a
`DSGLibrary`.  Every comparison is bit for bit unless it says otherwise: element b of a keyed batch against the batch-1 call after
`manual_seed(seed_b, stream_b)` with element b's conditioning, on a handle with the same kernel set named."""
import ctypes
import functools

import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
from diffusestylegesture_amd.model import ClassifierFreeSampleModel, DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.clip_init_util import clip_init
from tests.clip_inpaint_util import clip_constraint, n_out_of

STREAMS = (7, 0, 2 ** 33 + 5)          # the high word is used, one id is 0
SEEDS = (5, 6, 2 ** 40 + 1)
SHARED = 5                             # the seed of the calls whose elements share one
CLIPS = (10, 11, 12)                   # every clip its own conditioning
SKIP = 996                             # 1000 - 4: four steps
NOISE_TOL = 2e-6                       # tests/test_emu_round6.py::test_noise_stream_vs_oracle


@functools.lru_cache(maxsize=None)
def _sd(name):
    return synth_state_dict(getattr(C, name), 9)


def model(lib, cfg, prec, B, kset=None, **kw):
    m = DSGDenoiser(cfg, precision=prec, max_batch=B, library=lib, **kw)
    m.load_state_dict(_sd(cfg.name.upper()))
    if kset is not None:
        m.set_kernel_set(kset)
    return m


def accepted_sets(lib, cfg, prec, B):
    """the kernel sets a handle of these dims takes for batch B AND batch 1 (one set is named for both sides of every comparison)"""
    out = []
    for ks in ("latency", "tile", "block", "stream", "rows"):
        try:
            for b in (B, 1):
                m = model(lib, cfg, prec, b, ks)
                d = create_gaussian_diffusion(library=lib).manual_seed(1, 0)
                d.p_sample_loop(m, (b, cfg.njoints, 1, cfg.n_poses), clip_denoised=False, model_kwargs={"y": y_of(cfg, CLIPS[:b])},
                                skip_timesteps=d.num_timesteps - 1)
                assert m.last_kernel_set() == ks
        except (NotImplementedError, ValueError):
            continue
        out.append(ks)
    return out


def y_of(cfg, clips, window=1):
    return synth_window_inputs(cfg, len(clips), window=window, clips=list(clips), seed_pose_scale=0.3)


def y_slice(y, b):
    return {k: (v if k == "mask_local" else v[b:b + 1]) for k, v in y.items()}


def pairs(seeds, ids):
    return list(ids) if seeds is None else list(zip(seeds, ids))


def loop(d, ddim):
    return functools.partial(d.ddim_sample_loop, eta=0.5) if ddim else d.p_sample_loop


def diffusion(lib):
    return create_gaussian_diffusion(library=lib)


# ---- 1. the noise itself ----------------------------------------------------------------------------------------------------------------
def noise_streams(lib, B, J, T, seeds, ids, draw):
    out = np.zeros((B, J, 1, T), np.float32)
    u = [None if v is None else np.array(v, dtype=np.uint64) for v in (seeds, ids)]
    lib.check(lib.cdll.dsg_noise_streams(out.ctypes.data, B, J, T, *[None if a is None else a.ctypes.data for a in u], draw, None))
    return out


def noise_alone(lib, J, T, seed, sid, draw):
    out = np.zeros((1, J, 1, T), np.float32)
    lib.check(lib.cdll.dsg_noise(out.ctypes.data, 1, J, T, ctypes.c_uint64(seed), ctypes.c_uint64(sid), draw, None))
    return out


def check_noise(lib):
    from oracle import philox
    cfg = C.TINY
    J, T = cfg.njoints, cfg.n_poses
    for seeds in ((SHARED,) * 3, SEEDS):
        for draw in (0, 5):
            got = noise_streams(lib, 3, J, T, seeds, STREAMS, draw)
            for b in range(3):
                assert np.array_equal(got[b:b + 1], noise_alone(lib, J, T, seeds[b], STREAMS[b], draw)), (seeds, draw, b)
                want = philox.normal_bj1t((1, J, 1, T), seeds[b], draw, STREAMS[b])
                err = float(np.max(np.abs(got[b:b + 1] - want)))
                print(f"noise streams vs oracle: seeds {seeds} draw {draw} element {b}: max abs {err:.3e} (bound {NOISE_TOL})")
                assert err < NOISE_TOL
            assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])
    # a NULL array reads as zeros
    assert np.array_equal(noise_streams(lib, 3, J, T, None, STREAMS, 5), noise_streams(lib, 3, J, T, (0, 0, 0), STREAMS, 5))
    assert np.array_equal(noise_streams(lib, 3, J, T, SEEDS, None, 5), noise_streams(lib, 3, J, T, SEEDS, (0, 0, 0), 5))


# ---- 2. slot invariance ---------------------------------------------------------------------------------------------------------------
def _variant_kw(variant, cfg, y, B):
    """extra keywords / y entries of one variant, for the whole batch"""
    kw, skip = {}, SKIP
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    if variant == "init":            # init_image + skip_timesteps: the q_sample draw
        kw["init_image"] = (0.5 * np.random.default_rng(3).standard_normal(shape)).astype(np.float32)
    elif variant == "inpaint":       # a window-level constraint: every third feature, the second half of the window
        mask = np.zeros(shape, bool)
        mask[:, ::3, :, cfg.n_poses // 2:] = True
        y = dict(y, inpainting_mask=mask, inpainted_motion=(0.3 * np.random.default_rng(4).standard_normal(shape)).astype(np.float32))
    elif variant == "guided":
        y = dict(y, scale=np.array([2.5, 1.0, 0.5], np.float32)[:B])
    elif variant == "const":
        kw["const_noise"] = True
    return kw, y, skip


def _slice_kw(kw, b):
    return {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def check_slot_invariance(lib, cfg, prec, kset, variant="plain", ddim=False, seeds=None, B=3):
    """element b of the keyed batch == the batch-1 call after manual_seed(seed_b, stream_b); the clips in reverse order give the outputs in
    reverse order; the keyed result is not the unkeyed one"""
    guided = variant == "guided"
    clips = (CLIPS[0],) * B if variant == "const" else CLIPS[:B]
    mk = lambda n: (lambda m: ClassifierFreeSampleModel(m) if guided else m)(model(lib, cfg, prec, (2 if guided else 1) * n, kset))
    mB, m1 = mk(B), mk(1)
    d = diffusion(lib)
    kw, y, skip = _variant_kw(variant, cfg, y_of(cfg, clips), B)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    streams = pairs(seeds, STREAMS[:B])
    d.manual_seed(SHARED, 99)          # (the stream id of the call is ignored while the batch is keyed)
    got = np.asarray(loop(d, ddim)(mB, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip, clip_streams=streams, **kw))
    inner = mB.model if guided else mB
    assert inner.last_kernel_set() == kset and d._draw == 5 and inner.noise_streams is None      # (cleared after the call)
    for b in range(B):
        e = 0 if variant == "const" else b      # (const_noise: element 0's stream for everyone)
        d.manual_seed(SHARED if seeds is None else seeds[e], STREAMS[e])
        alone = np.asarray(loop(d, ddim)(m1, (1,) + shape[1:], clip_denoised=False, model_kwargs={"y": y_slice(y, b)}, skip_timesteps=skip,
                                         **_slice_kw(kw, b)))
        assert (m1.model if guided else m1).last_kernel_set() == kset
        assert np.array_equal(got[b:b + 1], alone), (cfg.name, prec, kset, variant, ddim, b, float(np.max(np.abs(got[b:b + 1] - alone))))
    if variant == "const":
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
        return
    # reversed order of the clips -> reversed outputs
    r = slice(None, None, -1)
    y_rev = {k: (v if k == "mask_local" else np.ascontiguousarray(v[r])) for k, v in y.items()}
    kw_rev = {k: (np.ascontiguousarray(v[r]) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    d.manual_seed(SHARED, 99)
    rev = np.asarray(loop(d, ddim)(mB, shape, clip_denoised=False, model_kwargs={"y": y_rev}, skip_timesteps=skip, clip_streams=streams[::-1],
                                   **kw_rev))
    assert np.array_equal(rev, got[r]), (cfg.name, prec, kset, variant)
    # and the streams matter: the same call unkeyed is another sample for the elements behind slot 0
    d.manual_seed(SHARED, STREAMS[0])
    plain = np.asarray(loop(d, ddim)(mB, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip, **kw))
    assert not np.array_equal(plain[1:], got[1:])
    if seeds is None:                  # (slot 0 of the call's own stream IS the batch-1 tensor of that stream)
        assert np.array_equal(plain[:1], got[:1])


# ---- 3. arrangement invariance ---------------------------------------------------------------------------------------------------------
def check_arrangements(lib, cfg, prec, kset):
    clips, ids = (10, 11, 12, 13), (7, 0, 2 ** 33 + 5, 9)
    d = diffusion(lib)
    base = model(lib, cfg, prec, 4, kset)
    per_clip = {}
    for n_lanes, B in ((1, 4), (2, 2), (4, 1)):
        lanes = [base] + [base.clone(B) for _ in range(n_lanes - 1)]      # (clones inherit the kernel set)
        ys = [{"y": y_of(cfg, clips[i * B:(i + 1) * B])} for i in range(n_lanes)]
        cs = [list(ids[i * B:(i + 1) * B]) for i in range(n_lanes)]
        d.manual_seed(SHARED, 0)
        outs = d.p_sample_loop_multi(lanes, (B, cfg.njoints, 1, cfg.n_poses), ys, skip_timesteps=SKIP, clip_streams=cs)
        assert all(ln.last_kernel_set() == kset and ln.noise_streams is None for ln in lanes) and d._draw == 5
        per_clip[n_lanes] = np.concatenate([np.asarray(o) for o in outs], 0)
    assert np.array_equal(per_clip[1], per_clip[2]) and np.array_equal(per_clip[1], per_clip[4])
    assert len({per_clip[1][c].tobytes() for c in range(4)}) == 4


# ---- 4. whole clips ------------------------------------------------------------------------------------------------------------------
def _clip_inputs(cfg, clips, K):
    zeggs = cfg is C.TINY
    feats = [synth_window_inputs(cfg if zeggs else C.TINY4, len(clips), window=w, clips=list(clips))["audio"] for w in range(K)]
    y0 = synth_window_inputs(cfg, len(clips), window=0, clips=list(clips), seed_pose_scale=0.3)
    return feats, y0["style"], y0["seed"]


def _gen(cfg, m, d, ins, windows, **kw):
    feats, style, seed_pose = ins
    if cfg is C.TINY:
        return S.generate_clip(m, d, feats, style, seed=SHARED, skip_timesteps=SKIP, seed_pose=seed_pose, windows=windows, **kw)
    return S.generate_clip_dsgplus(m, d, feats, style, seed_pose, len(feats) * cfg.stride, seed=SHARED, skip_timesteps=SKIP,
                                   feature_division=1, windows=windows, **kw)


def check_whole_clips(lib, cfg, prec, kset, Ks=(2, 3), variants=("plain", "init", "constraint")):
    B = 3
    klt = cfg is not C.TINY
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    for K in Ks:
        ins = _clip_inputs(cfg, CLIPS, K)
        for variant in variants:
            kw = {}
            if variant == "init":
                kw["init_motion"] = clip_init(cfg, B, K, klt)
            elif variant == "constraint":
                mask, motion, _ = clip_constraint(cfg, B, K, klt)
                kw.update(inpainting_mask=mask, inpainted_motion=motion)
            host = _gen(cfg, mB, d, ins, "host", clip_ids=STREAMS, **kw)
            assert d._draw == K * 5                                   # K * (1 + n_run), as before
            lib_ = _gen(cfg, mB, d, ins, "library", clip_ids=STREAMS, **kw)
            assert d._draw == K * 5 and mB.noise_streams is None and not mB.clip_init and not mB.clip_inpainting
            assert host.shape == (B, n_out_of(cfg, K, klt), cfg.njoints) and np.array_equal(host, lib_), (cfg.name, K, variant)
            for b in range(B):
                ins1 = ([f[b:b + 1] for f in ins[0]], ins[1][b:b + 1], ins[2][b:b + 1])
                alone = _gen(cfg, m1, d, ins1, "host" if b else "library", stream_id=STREAMS[b], **{k: v[b:b + 1] for k, v in kw.items()})
                assert np.array_equal(host[b:b + 1], alone), (cfg.name, prec, kset, K, variant, b)


# ---- 6. off is off ----------------------------------------------------------------------------------------------------------------------
def check_off_is_off(lib, cfg, prec, kset):
    B = 3
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    y = y_of(cfg, CLIPS)
    d = diffusion(lib)
    run = lambda m, **kw: np.asarray(d.manual_seed(SHARED, 3).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y},
                                                                             skip_timesteps=SKIP, **kw))
    m = model(lib, cfg, prec, B, kset)
    m.set_noise_streams(SEEDS, STREAMS)
    assert m.noise_streams == (list(SEEDS), list(STREAMS))
    lane = m.clone()                                   # a clone of a keyed handle starts unkeyed
    assert lane.noise_streams is None
    fresh = run(model(lib, cfg, prec, B, kset))
    assert np.array_equal(run(lane), fresh)
    # sticky: a dsg_sample straight on the keyed handle draws the streams
    d.manual_seed(SHARED, 3)
    a_, keep, _, _ = d._prepare(L.MODE_DDPM, m, False, shape, None, {"y": y}, SKIP, None, None, False, 0.0, None, None, None, False)
    sticky = np.empty(shape, np.float32)
    lib.check(lib.cdll.dsg_sample(m.handle, ctypes.byref(a_), sticky.ctypes.data, B, None))
    keyed = run(m, clip_streams=pairs(SEEDS, STREAMS))
    assert np.array_equal(sticky, keyed) and not np.array_equal(keyed, fresh)
    assert m.noise_streams is None                     # (the loop clears what it set)
    assert np.array_equal(run(m), fresh)               # set, sample, clear, sample: a fresh handle's bits


# ---- 7. generators own their streams ------------------------------------------------------------------------------------------------
def check_generators(lib, cfg, prec, kset):
    B = 3
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    y = y_of(cfg, CLIPS)
    m, d = model(lib, cfg, prec, B, kset), diffusion(lib)
    d.PROGRESSIVE_CHUNK = 3                            # 4 steps in two library calls: a manual_seed between the chunks as well
    for cs in (None, pairs(SEEDS, STREAMS)):
        gen = lambda: d.p_sample_loop_progressive(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP, clip_streams=cs)
        want = [np.asarray(o["sample"]) for o in d.manual_seed(11, 4) and gen()]
        g = d.manual_seed(11, 4) and gen()
        d.manual_seed(12, 8)                           # between creation and the first next()
        got = [np.asarray(next(g)["sample"])]
        d.manual_seed(13, 9)                           # between two chunks
        got += [np.asarray(o["sample"]) for o in g]
        assert len(got) == len(want) == 4 and all(np.array_equal(a, b) for a, b in zip(got, want)), cs
        assert m.noise_streams is None
        one = np.asarray(d.manual_seed(11, 4).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP,
                                                            clip_streams=cs))
        assert np.array_equal(one, want[-1])
        # a loop started after the manual_seed draws the other stream's noise
        other = np.asarray(d.manual_seed(12, 8).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP))
        g = d.manual_seed(11, 4) and gen()
        d.manual_seed(12, 8)
        list(g)
        after = np.asarray(d.p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP))
        assert np.array_equal(after, other) and not np.array_equal(after, want[-1])


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def check_errors(lib, cfg):
    import pytest
    B = 3
    m, d = model(lib, cfg, "fp32", B), diffusion(lib)
    y = y_of(cfg, CLIPS)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    u = np.array([1, 2, 3, 4], dtype=np.uint64)
    # B > max_batch, B < 1
    for n in (4, 0):
        assert lib.cdll.dsg_set_noise_streams(m.handle, u.ctypes.data, u.ctypes.data, n) == L.E_INVALID
    with pytest.raises(ValueError, match="max_batch"):
        m.set_noise_streams([1, 2, 3, 4], [1, 2, 3, 4])
    assert m.noise_streams is None
    # B mismatch at the sampling call, both numbers in the message
    m.set_noise_streams(None, [1, 2])
    with pytest.raises(ValueError, match=r"batch 3 .*\(2\)"):
        a, keep, _, _ = d._prepare(L.MODE_DDPM, m, False, shape, None, {"y": y}, SKIP, None, None, False, 0.0, None, None, None, False)
        out = np.empty(shape, np.float32)
        lib.check(lib.cdll.dsg_sample(m.handle, ctypes.byref(a), out.ctypes.data, B, None))
    m.set_noise_streams(None, None)
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        d.p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP, clip_streams=[1, 2])
    with pytest.raises(ValueError):
        d.p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP, clip_streams=[1, (2, 3), 4])
    # per lane: the number of lists, and a list's length
    lane = m.clone()
    with pytest.raises(ValueError, match="1 lists for 2 lanes"):
        d.p_sample_loop_multi([m, lane], shape, [{"y": y}] * 2, skip_timesteps=SKIP, clip_streams=[[1, 2, 3]])
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        d.p_sample_loop_multi([m, lane], shape, [{"y": y}] * 2, skip_timesteps=SKIP, clip_streams=[[1, 2, 3], [4, 5]])
    assert m.noise_streams is None and lane.noise_streams is None
    # the clip drivers: clip_ids together with a stream id; a wrong list length per lane
    ins = _clip_inputs(cfg, CLIPS, 2)
    for windows in ("host", "library"):
        with pytest.raises(ValueError, match="exclude"):
            _gen(cfg, m, d, ins, windows, clip_ids=STREAMS, stream_id=0)
        with pytest.raises(ValueError, match="2 entries for a batch of 3"):
            _gen(cfg, m, d, ins, windows, clip_ids=STREAMS[:2])
        feats, style, _ = ins
        with pytest.raises(ValueError, match="exclude"):
            S.generate_clips_streams([m, lane], d, [feats, feats], style, seed=SHARED, skip_timesteps=SKIP, stream_ids=[0, 1],
                                     clip_ids=[STREAMS, STREAMS], kernel_set=None, windows=windows)
        with pytest.raises(ValueError, match="entries for a batch of 3"):
            S.generate_clips_streams([m, lane], d, [feats, feats], style, seed=SHARED, skip_timesteps=SKIP,
                                     clip_ids=[STREAMS, STREAMS[:2]], kernel_set=None, windows=windows)
        with pytest.raises(ValueError, match="1 lists for 2 lanes"):
            S.generate_clips_streams([m, lane], d, [feats, feats], style, seed=SHARED, skip_timesteps=SKIP, clip_ids=[STREAMS],
                                     kernel_set=None, windows=windows)
