"""CPU: motion inpainting over a whole clip (dsg_set_clip_inpainting; `inpainting_mask` / `inpainted_motion` of the clip drivers and of
DSGDiffusion.sample_clip) through the product sources under the SIMT emulator: the cut kernel (k_clip_inp_window), its sequencing between the
step loops of dsg_sample_clip, and the Python routing -- bit for bit against the host window loop with `sample.window_constraint(...)` in y,
exactly where the mask is set, and against the oracle's inference() loops with the constraint as their denoised_fn.  The real-hardware tests
are tests/test_gpu_clip_inpaint.py (-m gpu)."""
import ctypes
import functools

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
from diffusestylegesture_amd.model import ClassifierFreeSampleModel, DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.clip_inpaint_util import MASK_KINDS, clip_constraint, n_out_of, window_constraint_by_index
from tests.util import rel_l2

TOL_CHAIN_FP32 = 3 * 1e-5      # the emulator's fp32 chain bound, as tests/test_emu_clip.py:18
SKIP = 996                     # 1000 - 4: four steps per window
CFGS = [C.TINY, C.TINY4, C.TINY5, C.TINY3B]


@functools.lru_cache(maxsize=None)
def _sd(name):
    return synth_state_dict(getattr(C, name), 9)


def _model(emu_lib, cfg, prec, B):
    m = DSGDenoiser(cfg, precision=prec, max_batch=B, library=emu_lib)
    m.load_state_dict(_sd(cfg.name.upper()))
    return m


def _inputs(cfg, B, K, clip0=0):
    zeggs = cfg is C.TINY
    feats = [synth_window_inputs(cfg if zeggs else C.TINY4, B, window=w, clip0=clip0)["audio"] for w in range(K)]
    y0 = synth_window_inputs(cfg, B, window=0, clip0=clip0, seed_pose_scale=0.3)
    return feats, y0["style"], y0["seed"], y0.get("seed_last")


def _clip(cfg, m, d, ins, windows, con=None, smoothing=True, ddim=False, eta=0.0, seed=5, stream_id=0, skip=None, seed0=True):
    """the clip drivers of sample.py; `con` = (mask, motion) in the coordinates of the returned clip; `seed0=False`: the ZEGGS loop
    starts from a zero seed (sample.py:241)"""
    feats, style, seed_pose, seed_last = ins
    kw = {} if con is None else dict(inpainting_mask=con[0], inpainted_motion=con[1])
    skip = (d.num_timesteps - 4) if skip is None else skip
    if cfg is C.TINY:
        return S.generate_clip(m, d, feats, style, seed=seed, smoothing=smoothing, skip_timesteps=skip, stream_id=stream_id,
                               seed_pose=seed_pose if seed0 else None, windows=windows, ddim=ddim, eta=eta, **kw)
    return S.generate_clip_dsgplus(m, d, feats, style, seed_pose, len(feats) * cfg.stride, seed=seed, skip_timesteps=skip, stream_id=stream_id,
                                   seed_last=seed_last, feature_division=1, windows=windows, ddim=ddim, eta=eta, **kw)


def _con(cfg, B, K, first=0):
    mask, motion, kinds = clip_constraint(cfg, B, K, cfg is not C.TINY, first=first)
    return (mask, motion), kinds


# ---- 1. bit identity, library against host loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: c.name)
def test_library_windows_bit_identical_to_host_loop(emu_lib, cfg, prec):
    """K = 1 (no hand-off: the first S frames and the cut tail are unconstrained), 2, 3; B = 1 and 3 clips with a different mask each"""
    d = create_gaussian_diffusion(library=emu_lib)
    for B in (1, 3):
        m = _model(emu_lib, cfg, prec, B)
        for K in (1, 2, 3):
            ins = _inputs(cfg, B, K, clip0=B)
            con, kinds = _con(cfg, B, K, first=K)           # (B = 1: another kind of mask for every K)
            host = _clip(cfg, m, d, ins, "host", con)
            draw_host, ks, path = d._draw, m.last_kernel_set(), m.last_sample_path()
            assert not m.inpainting and not m.clip_inpainting      # (the host form leaves no window-level constraint behind)
            lib = _clip(cfg, m, d, ins, "library", con)
            assert host.shape == lib.shape == con[1].shape == (B, n_out_of(cfg, K, cfg is not C.TINY), cfg.njoints)
            assert np.array_equal(host, lib), (B, K, kinds)
            assert d._draw == draw_host == K * 5 and m.last_sample_ms()[1] == K * 4
            assert m.last_kernel_set() == ks and m.last_sample_path() == path
            assert not m.clip_inpainting                     # (cleared after the call)
            assert not np.array_equal(lib, _clip(cfg, m, d, ins, "library")), (B, K)      # (the constraint does something)


# ---- 2. the constraint holds exactly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,smoothing", [(C.TINY, False), (C.TINY, True), (C.TINY4, False), (C.TINY5, False)],
                         ids=["tiny-noshift", "tiny-rootshift", "tiny4", "tiny5"])
def test_constraint_holds_exactly(emu_lib, cfg, smoothing):
    """DDPM, clip_denoised=False: at loop index 0 the posterior mean IS x0 and no noise is added (tests/test_emu_inpaint.py:45-57), the blend of
    two equal values returns the value.  With the root shift: features >= 3 always; features < 3 too where the hand-off frames are constrained
    (mask "frames": the shift delta of a constrained root channel is 0 there, for every window)."""
    B, K = 3, 3
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion(library=emu_lib)
    (mask, motion), kinds = _con(cfg, B, K)
    out = _clip(cfg, m, d, _inputs(cfg, B, K), "library", (mask, motion), smoothing=smoothing)
    on = mask != 0
    if not smoothing:
        assert np.array_equal(out[on], motion[on])
    else:
        assert np.array_equal(out[..., 3:][on[..., 3:]], motion[..., 3:][on[..., 3:]])
        b = kinds.index("frames")
        assert on[b, :, :3].any() and np.array_equal(out[b][on[b]], motion[b][on[b]])
        b = kinds.index("checker")                           # (and a root channel that is free at a hand-off frame IS moved)
        assert not np.array_equal(out[b, :, :3][on[b, :, :3]], motion[b, :, :3][on[b, :, :3]])
    assert not np.array_equal(out[~on], motion[~on])


def test_constraint_then_clamp(emu_lib):
    """clip_denoised=True: the constraint first, then the clamp -- np.clip(motion, -1, 1) where the mask is set"""
    cfg, B, K = C.TINY, 3, 3
    m, d = _model(emu_lib, cfg, "fp32", B), create_gaussian_diffusion(library=emu_lib)
    feats, style, seed_pose, _ = _inputs(cfg, B, K)
    (mask, motion), _ = _con(cfg, B, K)
    out = d.manual_seed(5, 0).sample_clip(m, feats, style, seed0=seed_pose, root_shift=False, keep_last_tail=False, skip_timesteps=SKIP,
                                          clip_denoised=True, inpainting_mask=mask, inpainted_motion=motion)
    on = mask != 0
    assert (np.abs(motion[on]) > 1).any() and np.array_equal(out[on], np.clip(motion, -1, 1)[on])


# ---- 3. the cut kernel alone ------------------------------------------------------------------------------------------------------
def _numpy_stitch(cfg, K, sample_window, tail):
    """tests/test_gpu_clip.py:105-133: the K single-window samples stitched by a numpy restatement of sample.py:269-289 / BEAT-TWH
    sample.py:150-160 (fp32, the same operations in the same order); sample_window(c, seed [B, J, 1, S]) -> [B, J, 1, T]"""
    zeggs = cfg is C.TINY
    Sd, T = cfg.n_seed, cfg.n_poses
    rows = []
    for c in range(K):
        s = np.asarray(sample_window(c, np.ascontiguousarray(tail)))[:, :, 0, :].transpose(0, 2, 1).copy()      # [B, T, J]
        if c > 0:
            last0 = tail[:, :, 0, 0]
            if zeggs:
                delta = s[:, 0, :3] - last0[:, :3]
                s[:, :, :3] = s[:, :, :3] - delta[:, None, :]
            s[:, 0] = last0 * np.float32(0.5) + s[:, 0] * np.float32(0.5)
        tail = s[:, T - Sd:].transpose(0, 2, 1)[:, :, None, :]
        rows.append(s if (c == K - 1 and not zeggs) else s[:, : T - Sd])
    return np.concatenate(rows, 1)[:, Sd:]


@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_cut_kernel_alone_vs_numpy_stitch(emu_lib, cfg):
    """one step per window: the clip call is the cut kernel, one pose head and the hand-off.  Yardstick: K p_sample_loop calls with
    y['inpainting_*'] = window_constraint(...), stitched in numpy"""
    B, K = 3, 3
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion(library=emu_lib)
    skip = d.num_timesteps - 1
    ins = _inputs(cfg, B, K)
    feats, style, seed_pose, _ = ins
    (mask, motion), _ = _con(cfg, B, K)
    klt = cfg is not C.TINY
    got = _clip(cfg, m, d, ins, "library", (mask, motion), skip=skip)
    d.manual_seed(5, 0)

    def sample_window(c, seed):
        wm, wv = S.window_constraint(cfg, mask, motion, c, klt)
        y = {"style": style, "seed": seed, "audio": feats[c], "mask_local": np.ones((1, cfg.n_poses), bool), "inpainting_mask": wm, "inpainted_motion": wv}
        return d.p_sample_loop(m, (B, cfg.njoints, 1, cfg.n_poses), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip)
    want = _numpy_stitch(cfg, K, sample_window, seed_pose)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_window_constraint_vs_index_loop(cfg):
    for klt in (False, True):
        for K in (1, 2, 3):
            mask, motion, _ = clip_constraint(cfg, 3, K, klt)
            seen = np.zeros(mask.shape, int)
            for c in range(K):
                wm, wv = S.window_constraint(cfg, mask, motion, c, klt)
                im, iv = window_constraint_by_index(cfg, mask, motion, c)
                assert wm.dtype == np.bool_ and wv.dtype == np.float32 and wm.shape == wv.shape == (3, cfg.njoints, 1, cfg.n_poses)
                assert np.array_equal(wm, im) and np.array_equal(wv, iv)
                lo = c * cfg.stride - cfg.n_seed
                seen[:, max(lo, 0): lo + cfg.n_poses] += 1
            # every clip row belongs to a window; the S rows behind every hand-off to two
            assert seen.min() == 1 and np.count_nonzero(seen[0, :, 0] == 2) == (K - 1) * cfg.n_seed
            with pytest.raises(ValueError):
                S.window_constraint(cfg, mask, motion, K, klt)
            with pytest.raises(ValueError):
                S.window_constraint(cfg, mask[:, :-1], motion[:, :-1], 0, klt)
    import torch
    tm, tv = S.window_constraint(cfg, torch.from_numpy(mask), torch.from_numpy(motion), 1, True)
    im, iv = window_constraint_by_index(cfg, mask, motion, 1)
    assert tm.dtype == torch.bool and np.array_equal(tm.numpy(), im) and np.array_equal(tv.numpy(), iv)


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: c.name)
def test_vs_oracle(emu_lib, cfg):
    """the oracle's inference() loops with denoised_fn = the window's constraint (tests/test_inpaint_golden.py: inpaint_fn, pinned to the
    reference by G18), fp32, rel-L2 over the unmasked elements of one clip -- one clip per kind of mask.  Measured: 3.2e-7 .. 1.1e-6 (bound 3e-5)"""
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    from tests.test_inpaint_golden import inpaint_fn
    B, K, seed, sid = 3, 3, 5, 2
    klt = cfg is not C.TINY
    m, d = _model(emu_lib, cfg, "fp32", B), create_gaussian_diffusion(library=emu_lib)
    ins = _inputs(cfg, B, K)
    feats, style, seed_pose, seed_last = ins
    (mask, motion), kinds = _con(cfg, B, K)
    got = _clip(cfg, m, d, ins, "library", (mask, motion), seed=seed, stream_id=sid, seed0=False)
    ref, od = MDMOracle(_sd(cfg.name.upper()), cfg), OracleDiffusion()
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    Jc = cfg.njoints if cfg is C.TINY else cfg.njoints // 3          # (dsgplus_clip keeps the first J/3 features)
    for b, kind in enumerate(kinds):
        def sample_window(c, yy):
            nf = lambda k: philox.normal_bj1t(shape, seed, c * 5 + k, sid)[b:b + 1]
            wm, wv = S.window_constraint(cfg, mask[b:b + 1], motion[b:b + 1], c, klt)
            return sampler.p_sample_loop(od, ref, (1,) + shape[1:], nf, {"y": yy}, skip_timesteps=SKIP, denoised_fn=inpaint_fn(wm, wv))
        fb = [f[b:b + 1] for f in feats]
        if cfg is C.TINY:
            want = sampler.zeggs_clip(sample_window, cfg, fb, list(style[b]), smoothing=True)
        else:
            want = sampler.dsgplus_clip(sample_window, cfg, fb, list(style[b]), seed_pose[b:b + 1], K * cfg.stride,
                                        seed_last=None if seed_last is None else seed_last[b:b + 1])
        g, free = got[b][:, :Jc], mask[b][:, :Jc] == 0
        assert g.shape == want.shape and np.count_nonzero(free) >= free.size // 4      # (the DSG+ crop to J/3 features keeps 3 free columns of "block")
        e = rel_l2(g[free], want[free])
        print(cfg.name, kind, "constrained library clip vs oracle, unmasked elements", e)
        assert e < TOL_CHAIN_FP32


# ---- 5. DDIM and guidance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim(emu_lib, cfg, eta):
    B, K = 3, 3
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion("ddim50", library=emu_lib)
    ins = _inputs(cfg, B, K)
    (mask, motion), _ = _con(cfg, B, K)
    host = _clip(cfg, m, d, ins, "host", (mask, motion), ddim=True, eta=eta)
    draw_host = d._draw
    lib = _clip(cfg, m, d, ins, "library", (mask, motion), ddim=True, eta=eta)
    assert np.array_equal(host, lib) and d._draw == draw_host == K * 5
    on = (mask != 0)[..., 3:]                    # alphas_cumprod_prev[0] == 1: the last DDIM step returns x0
    assert np.array_equal(lib[..., 3:][on], motion[..., 3:][on])


def test_guided(emu_lib):
    """classifier-free guidance: the host loop of sample.py written out with y['scale'] and the window's constraint, against sample_clip;
    the constraint acts on the COMBINED prediction, so it holds exactly"""
    cfg, B, K = C.TINY, 2, 3
    m, d = ClassifierFreeSampleModel(_model(emu_lib, cfg, "bf16", 2 * B)), create_gaussian_diffusion(library=emu_lib)
    feats, style, seed_pose, _ = _inputs(cfg, B, K)
    (mask, motion), _ = _con(cfg, B, K, first=1)
    scale = np.array([2.5, 0.5], np.float32)
    out = []
    d.manual_seed(11, 3)
    for c, feat in enumerate(feats):
        y = S._zeggs_window_y(cfg, feat, style, out[-1] if out else None, seed_pose, False, np.ones((1, cfg.n_poses), bool))
        wm, wv = S.window_constraint(cfg, mask, motion, c, False)
        s = d.p_sample_loop(m, (B, cfg.njoints, 1, cfg.n_poses), clip_denoised=False, skip_timesteps=SKIP,
                            model_kwargs={"y": dict(y, scale=scale, inpainting_mask=wm, inpainted_motion=wv)})
        S._zeggs_stitch(out, s, cfg.n_seed, True, False)
    host = S._zeggs_finish(out, cfg.n_seed, False)
    draw_host = d._draw
    m.model.set_inpainting(None, None, 0)           # (the last window's constraint is sticky on the lane; the clip call refuses one)
    kw = dict(seed0=seed_pose, root_shift=True, keep_last_tail=False, skip_timesteps=SKIP, inpainting_mask=mask, inpainted_motion=motion)
    lib = d.manual_seed(11, 3).sample_clip(m, feats, style, scale=scale, **kw)
    assert np.array_equal(host, lib) and d._draw == draw_host
    on = (mask != 0)[..., 3:]
    assert np.array_equal(lib[..., 3:][on], motion[..., 3:][on])
    assert not np.array_equal(d.manual_seed(11, 3).sample_clip(m.model, feats, style, **kw), lib)      # (guidance does something)


# ---- 6. lanes ---------------------------------------------------------------------------------------------------------------------------
def test_lanes(emu_lib):
    """two lanes x 2 clips, lane 0 constrained, lane 1 not: each lane bit-identical to the same lane run alone, lane 1 to a run with no
    constraint anywhere; the host form of the multi-lane drivers agrees"""
    for cfg in (C.TINY, C.TINY5):
        B, K, NL = 2, 3, 2
        m = _model(emu_lib, cfg, "bf16", B)
        lanes, d = [m, m.clone()], create_gaussian_diffusion(library=emu_lib)
        per = [_inputs(cfg, B, K, clip0=ln * B) for ln in range(NL)]
        feats = [p[0] for p in per]
        (mask, motion), _ = _con(cfg, B, K, first=1)

        def run(w, masks, motions):
            kw = dict(seed=7, skip_timesteps=SKIP, stream_ids=[3, 4], kernel_set=None, windows=w, inpainting_mask=masks, inpainted_motion=motions)
            if cfg is C.TINY:
                return S.generate_clips_streams(lanes, d, feats, per[0][1], **kw)
            return S.generate_clips_streams_dsgplus(lanes, d, feats, per[0][1], [p[2] for p in per], K * cfg.stride, seed_lasts=[p[3] for p in per],
                                                    feature_division=1, **kw)
        lib = run("library", [mask, None], [motion, None])
        assert lib.shape[0] == NL * B and np.array_equal(run("host", [mask, None], [motion, None]), lib)
        free = run("library", None, None)
        assert np.array_equal(lib[B:], free[B:]) and not np.array_equal(lib[:B], free[:B])
        assert not lanes[0].clip_inpainting and not lanes[1].clip_inpainting
        for ln in range(NL):
            feats_l, style_l, seed_l, last_l = per[ln]
            kw = dict(seed=7, skip_timesteps=SKIP, stream_id=3 + ln, windows="library")
            if ln == 0:
                kw.update(inpainting_mask=mask, inpainted_motion=motion)
            if cfg is C.TINY:
                alone = S.generate_clip(lanes[ln], d, feats_l, per[0][1], **kw)
            else:
                alone = S.generate_clip_dsgplus(lanes[ln], d, feats_l, per[0][1], seed_l, K * cfg.stride, seed_last=last_l, feature_division=1, **kw)
            assert np.array_equal(alone, lib[ln * B:(ln + 1) * B]), (cfg.name, ln)
        with pytest.raises(ValueError):
            run("library", [mask, None], [None, motion])
        with pytest.raises(ValueError):
            run("host", [mask], [motion])


# ---- 7. stickiness and refusals -----------------------------------------------------------------------------------------------------
def test_stickiness_and_refusals(emu_lib):
    cfg, B, K = C.TINY, 2, 2
    m, d = _model(emu_lib, cfg, "fp32", B + 1), create_gaussian_diffusion(library=emu_lib)
    ins = _inputs(cfg, B, K)
    feats, style, seed_pose, _ = ins
    (mask, motion), _ = _con(cfg, B, K, first=1)
    n_out = n_out_of(cfg, K, False)
    free = _clip(cfg, m, d, ins, "library")
    held = _clip(cfg, m, d, ins, "library", (mask, motion))
    assert not np.array_equal(free, held)
    m.set_schedule(d)
    audio, sty, seed0 = L.Buf(np.stack(feats)), L.Buf(style), L.Buf(seed_pose)
    ones = L.Buf(np.ones((1, cfg.n_poses), np.uint8), "uint8")
    out = np.zeros((B, n_out, cfg.njoints), np.float32)

    def call(k=K, batch=B, o=out):
        a = L.dsg_sample_args()
        a.mode, a.skip_timesteps, a.seed = L.MODE_DDPM, SKIP, 5
        return emu_lib.cdll.dsg_sample_clip(m.handle, sty.p, seed0.p, audio.p, ones.p, 1, None, ctypes.byref(a), k, 1, 0, o.ctypes.data, batch, None)
    err = lambda: emu_lib.cdll.dsg_last_error().decode()
    # sticky: two calls in a row honour it; after set_clip_inpainting(None, None, 0) the clip is the unconstrained one, bit for bit
    m.set_clip_inpainting(mask, motion, B)
    assert m.clip_inpainting
    for _ in range(2):
        out[:] = 0
        assert call() == 0 and np.array_equal(out, held)
    # dsg_sample ignores it (and leaves it alone)
    y = synth_window_inputs(cfg, B, window=0, seed_pose_scale=0.3)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    one = d.manual_seed(9, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP)
    fresh = d.manual_seed(9, 1).p_sample_loop(_model(emu_lib, cfg, "fp32", B + 1), shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP)
    assert np.array_equal(one, fresh) and m.clip_inpainting
    assert call() == 0 and np.array_equal(out, held)
    # n_frames != n_out (another K), another batch: DSG_E_INVALID with both numbers in the message
    big = np.zeros((B, n_out_of(cfg, K + 1, False), cfg.njoints), np.float32)
    assert call(k=K + 1, o=big) == -1 and str(n_out) in err() and str(big.shape[1]) in err()
    f8 = np.ascontiguousarray(np.stack([np.concatenate([f, f[:1]]) for f in feats]))      # (B + 1 clips of features)
    a3, s3, p3 = L.Buf(f8), L.Buf(np.concatenate([style, style[:1]])), L.Buf(np.concatenate([seed_pose, seed_pose[:1]]))
    o3 = np.zeros((B + 1, n_out, cfg.njoints), np.float32)
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps, a.seed = L.MODE_DDPM, SKIP, 5
    assert emu_lib.cdll.dsg_sample_clip(m.handle, s3.p, p3.p, a3.p, ones.p, 1, None, ctypes.byref(a), K, 1, 0, o3.ctypes.data, B + 1, None) == -1
    assert str(B) in err() and str(B + 1) in err()
    assert call() == 0 and np.array_equal(out, held)          # (a refused call leaves the constraint as it was)
    # the setter through the bare ABI: exactly one NULL, B > max_batch, n_frames < 1
    f = emu_lib.cdll.dsg_set_clip_inpainting
    mb, vb = L.Buf(mask, "uint8"), L.Buf(motion)
    assert f(m.handle, mb.p, None, B, n_out, None) == -1 and err()
    assert f(m.handle, None, vb.p, B, n_out, None) == -1 and err()
    assert f(m.handle, mb.p, vb.p, B + 2, n_out, None) == -1 and err()
    assert f(m.handle, mb.p, vb.p, B, 0, None) == -1 and err()
    assert call() == 0 and np.array_equal(out, held)          # (refused settings left it alone too)
    # a window-level constraint is still refused by the clip call, with or without a clip-level one
    wm, wv = S.window_constraint(cfg, mask, motion, 0, False)
    m.set_inpainting(wm, wv, B)
    assert call() == -1 and "per window" in err()
    m.set_inpainting(None, None, 0)
    assert call() == 0 and np.array_equal(out, held)
    # a clone starts without one
    c = m.clone()
    assert c.clip_inpainting is False
    assert np.array_equal(_clip(cfg, c, d, ins, "library"), free)
    # off: bit for bit the unconstrained clip; a grown constraint (more frames than before) replaces the copy
    m.set_clip_inpainting(None, None, 0)
    assert not m.clip_inpainting and call() == 0 and np.array_equal(out, free)
    (mask3, motion3), _ = _con(cfg, B, K + 1, first=1)
    m.set_clip_inpainting(mask3, motion3, B)
    assert call(k=K + 1, o=big) == 0
    on = (mask3 != 0)[..., 3:]
    assert np.array_equal(big[..., 3:][on], motion3[..., 3:][on])
    m.set_clip_inpainting(None, None, 0)
    # Python: one without the other, a wrong shape
    with pytest.raises(ValueError):
        _clip(cfg, m, d, ins, "library", (mask, None))
    with pytest.raises(ValueError):
        _clip(cfg, m, d, ins, "host", (None, motion))
    with pytest.raises(ValueError):
        d.sample_clip(m, feats, style, root_shift=True, keep_last_tail=False, skip_timesteps=SKIP, inpainted_motion=motion)
    with pytest.raises(ValueError, match="shape"):
        _clip(cfg, m, d, ins, "library", (mask[:, :-1], motion[:, :-1]))
    with pytest.raises(ValueError, match="shape"):
        m.set_clip_inpainting(mask[..., :-1], motion, B)
    assert not m.clip_inpainting and np.array_equal(_clip(cfg, m, d, ins, "library"), free)


def test_one_new_kernel_without_scratch(hip_lib_path):
    """the rebuilt code object: the cut kernel is there, once, with ScratchSize 0 (the register report is read as
    tests/test_emu_inpaint.py reads it)"""
    import re
    from tests.test_emu_inpaint import _resource_report
    text = _resource_report()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch)
    cut = [s for n, s in zip(names, scratch) if "k_clip_inp_window" in n]
    assert cut == [0]
