"""CPU: editing an existing clip in one library call (dsg_set_clip_init; `init_motion` of the clip drivers and of DSGDiffusion.sample_clip)
through the product sources under the SIMT emulator: the start kernel (k_clip_x_in: window cut + q_sample + state write), its place in
dsg_sample_clip, and the Python routing -- bit for bit against the host window loop with `sample.window_init(...)` as every window's
`init_image`, and against the oracle's inference() loops started from the same slices.  The real-hardware tests are
tests/test_gpu_clip_init.py (-m gpu)."""
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
from tests.clip_init_util import clip_init, numpy_stitch, window_init_by_index
from tests.clip_inpaint_util import clip_constraint, n_out_of
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


def _clip(cfg, m, d, ins, windows, init=None, con=None, smoothing=True, ddim=False, eta=0.0, seed=5, stream_id=0, skip=None, seed0=True):
    """the clip drivers of sample.py; `init` [B, n_out, J] in the coordinates of the returned clip; `seed0=False`: the ZEGGS loop starts
    from a zero seed (sample.py:241)"""
    feats, style, seed_pose, seed_last = ins
    kw = {} if init is None else dict(init_motion=init)
    if con is not None:
        kw.update(inpainting_mask=con[0], inpainted_motion=con[1])
    skip = (d.num_timesteps - 4) if skip is None else skip
    if cfg is C.TINY:
        return S.generate_clip(m, d, feats, style, seed=seed, smoothing=smoothing, skip_timesteps=skip, stream_id=stream_id,
                               seed_pose=seed_pose if seed0 else None, windows=windows, ddim=ddim, eta=eta, **kw)
    return S.generate_clip_dsgplus(m, d, feats, style, seed_pose, len(feats) * cfg.stride, seed=seed, skip_timesteps=skip, stream_id=stream_id,
                                   seed_last=seed_last, feature_division=1, windows=windows, ddim=ddim, eta=eta, **kw)


def _init(cfg, B, K):
    return clip_init(cfg, B, K, cfg is not C.TINY)


# ---- 1. bit identity, library against host loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,prec", [(c, p) for c in CFGS for p in ("fp32", "bf16")] + [(C.TINY, "bf16w2")],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_library_windows_bit_identical_to_host_loop(emu_lib, cfg, prec):
    """K = 1 (the seed frames in front AND the held closing row in one window), 2, 3; B = 1 and 3 clips with a different init each; on
    TINY with the caller's seed poses and with the zero seed (the df < 0 rule; the zero seed at B = 1).  Each (B, K, seed) is one host and
    one library clip; that the init and the seed frames matter is shown once per B, at the last K"""
    d = create_gaussian_diffusion(library=emu_lib)
    for B in (1, 3):
        m = _model(emu_lib, cfg, prec, B)
        for K in (1, 2, 3):
            ins = _inputs(cfg, B, K, clip0=B)
            init = _init(cfg, B, K)
            for seed0 in ((True, False) if cfg is C.TINY and B == 1 else (True,)):
                host = _clip(cfg, m, d, ins, "host", init, seed0=seed0)
                draw_host, ks, path = d._draw, m.last_kernel_set(), m.last_sample_path()
                lib = _clip(cfg, m, d, ins, "library", init, seed0=seed0)
                assert host.shape == lib.shape == init.shape == (B, n_out_of(cfg, K, cfg is not C.TINY), cfg.njoints)
                assert np.array_equal(host, lib), (B, K, seed0)
                assert d._draw == draw_host == K * 5 and m.last_sample_ms()[1] == K * 4
                assert m.last_kernel_set() == ks and m.last_sample_path() == path
                assert not m.clip_init                           # (cleared after the call)
                if seed0:
                    with_seed = lib
                elif K == 3:
                    assert not np.array_equal(lib, with_seed)    # (the seed frames in front of the clip are part of the start)
        assert not np.array_equal(with_seed, _clip(cfg, m, d, ins, "library")), B      # (the init does something)


# ---- 2. the kernel alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_start_kernel_alone_vs_numpy_stitch(emu_lib, cfg):
    """one step per window: the clip call is the start kernel, one pose head and the hand-off.  Yardstick: K p_sample_loop calls with
    init_image = window_init(...), stitched in numpy"""
    B, K = 3, 3
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion(library=emu_lib)
    skip = d.num_timesteps - 1
    ins = _inputs(cfg, B, K)
    feats, style, seed_pose, _ = ins
    init = _init(cfg, B, K)
    klt = cfg is not C.TINY
    got = _clip(cfg, m, d, ins, "library", init, skip=skip)
    d.manual_seed(5, 0)

    def sample_window(c, seed):
        y = {"style": style, "seed": seed, "audio": feats[c], "mask_local": np.ones((1, cfg.n_poses), bool)}
        return d.p_sample_loop(m, (B, cfg.njoints, 1, cfg.n_poses), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip,
                               init_image=S.window_init(cfg, init, seed_pose, c, klt))
    want = numpy_stitch(not klt, cfg.n_seed, cfg.n_poses, K, sample_window, seed_pose)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- 3. window_init against the index loop ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_window_init_vs_index_loop(cfg):
    B, Sd, T = 3, cfg.n_seed, cfg.n_poses
    seed0 = synth_window_inputs(cfg, B, window=0, seed_pose_scale=0.3)["seed"]
    for klt in (False, True):
        for K in (1, 2, 3):
            init = clip_init(cfg, B, K, klt)
            n_out = init.shape[1]
            seen = np.zeros(n_out, int)
            for c in range(K):
                for sp in (seed0, None):
                    w = S.window_init(cfg, init, sp, c, klt)
                    assert w.dtype == np.float32 and w.shape == (B, cfg.njoints, 1, T)
                    assert np.array_equal(w, window_init_by_index(cfg, init, sp, c))
                lo = c * cfg.stride - Sd
                seen[max(lo, 0): lo + T] += 1
                if c == 0:          # df < 0: y['seed'] of window 0, zeros without one
                    assert np.array_equal(S.window_init(cfg, init, seed0, 0, klt)[..., :Sd], seed0)
                    assert not S.window_init(cfg, init, None, 0, klt)[..., :Sd].any()
                if c == K - 1 and not klt:      # df >= n_out: the held closing row
                    assert np.array_equal(w[:, :, 0, T - Sd:], np.repeat(init[:, n_out - 1][:, :, None], Sd, 2))
            # every clip row is read by one window; the S rows behind every hand-off by two
            assert seen.min() == 1 and np.count_nonzero(seen == 2) == (K - 1) * Sd and seen.max() <= 2
            with pytest.raises(ValueError):
                S.window_init(cfg, init, seed0, K, klt)
            with pytest.raises(ValueError):
                S.window_init(cfg, init[:, :-1], seed0, 0, klt)
    import torch
    for sp in (seed0, None):
        tw = S.window_init(cfg, torch.from_numpy(init), None if sp is None else torch.from_numpy(sp), 0, True)
        assert tw.dtype == torch.float32 and np.array_equal(tw.numpy(), window_init_by_index(cfg, init, sp, 0))
    assert np.array_equal(S.window_init(cfg, torch.from_numpy(init), None, K - 1, True).numpy(), window_init_by_index(cfg, init, None, K - 1))


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: c.name)
def test_vs_oracle(emu_lib, cfg):
    """the oracle's inference() loops, every window started from init_image = window_init(...) of its own y['seed'], fp32, rel-L2 per
    clip.  Measured: 4.1e-7 .. 1.3e-6 (bound 3e-5)"""
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    B, K, seed, sid = 3, 3, 5, 2
    klt = cfg is not C.TINY
    m, d = _model(emu_lib, cfg, "fp32", B), create_gaussian_diffusion(library=emu_lib)
    ins = _inputs(cfg, B, K)
    feats, style, seed_pose, seed_last = ins
    init = _init(cfg, B, K)
    got = _clip(cfg, m, d, ins, "library", init, seed=seed, stream_id=sid, seed0=False)
    ref, od = MDMOracle(_sd(cfg.name.upper()), cfg), OracleDiffusion()
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    Jc = cfg.njoints if cfg is C.TINY else cfg.njoints // 3          # (dsgplus_clip keeps the first J/3 features)
    for b in range(B):
        def sample_window(c, yy):
            nf = lambda k: philox.normal_bj1t(shape, seed, c * 5 + k, sid)[b:b + 1]
            wi = S.window_init(cfg, init, None if cfg is C.TINY else seed_pose, c, klt)
            return sampler.p_sample_loop(od, ref, (1,) + shape[1:], nf, {"y": yy}, skip_timesteps=SKIP, init_image=wi[b:b + 1])
        fb = [f[b:b + 1] for f in feats]
        if cfg is C.TINY:
            want = sampler.zeggs_clip(sample_window, cfg, fb, list(style[b]), smoothing=True)
        else:
            want = sampler.dsgplus_clip(sample_window, cfg, fb, list(style[b]), seed_pose[b:b + 1], K * cfg.stride,
                                        seed_last=None if seed_last is None else seed_last[b:b + 1])
        g = got[b][:, :Jc]
        assert g.shape == want.shape
        e = rel_l2(g, want)
        print(cfg.name, "clip", b, "library clip from an init motion vs oracle", e)
        assert e < TOL_CHAIN_FP32


# ---- 5. DDIM, 6. guidance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim(emu_lib, cfg, eta):
    B, K = 3, 3
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion("ddim50", library=emu_lib)
    ins = _inputs(cfg, B, K)
    init = _init(cfg, B, K)
    host = _clip(cfg, m, d, ins, "host", init, ddim=True, eta=eta)
    draw_host = d._draw
    lib = _clip(cfg, m, d, ins, "library", init, ddim=True, eta=eta)
    assert np.array_equal(host, lib) and d._draw == draw_host == K * 5
    assert not np.array_equal(lib, _clip(cfg, m, d, ins, "library", ddim=True, eta=eta))


def test_guided(emu_lib):
    """classifier-free guidance: the host loop of sample.py written out with y['scale'] and the window's init_image, against sample_clip;
    the unconditional twins must receive the same start"""
    cfg, B, K = C.TINY, 2, 3
    m, d = ClassifierFreeSampleModel(_model(emu_lib, cfg, "bf16", 2 * B)), create_gaussian_diffusion(library=emu_lib)
    feats, style, seed_pose, _ = _inputs(cfg, B, K)
    init = _init(cfg, B, K)
    scale = np.array([2.5, 0.5], np.float32)
    out = []
    d.manual_seed(11, 3)
    for c, feat in enumerate(feats):
        y = S._zeggs_window_y(cfg, feat, style, out[-1] if out else None, seed_pose, False, np.ones((1, cfg.n_poses), bool))
        s = d.p_sample_loop(m, (B, cfg.njoints, 1, cfg.n_poses), clip_denoised=False, skip_timesteps=SKIP, model_kwargs={"y": dict(y, scale=scale)},
                            init_image=S.window_init(cfg, init, seed_pose, c, False))
        S._zeggs_stitch(out, s, cfg.n_seed, True, False)
    host = S._zeggs_finish(out, cfg.n_seed, False)
    draw_host = d._draw
    kw = dict(seed0=seed_pose, root_shift=True, keep_last_tail=False, skip_timesteps=SKIP, init_motion=init)
    lib = d.manual_seed(11, 3).sample_clip(m, feats, style, scale=scale, **kw)
    assert np.array_equal(host, lib) and d._draw == draw_host
    assert not np.array_equal(d.manual_seed(11, 3).sample_clip(m.model, feats, style, **kw), lib)      # (guidance does something)
    kw.pop("init_motion")
    assert not np.array_equal(d.manual_seed(11, 3).sample_clip(m, feats, style, scale=scale, **kw), lib)      # (and so does the init)


# ---- 7. with the clip constraint ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_with_clip_constraint(emu_lib, cfg):
    """init and constraint together: library == host loop, and the constraint still holds exactly (features >= 3 under the root shift)"""
    B, K = 3, 3
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion(library=emu_lib)
    ins = _inputs(cfg, B, K)
    init = _init(cfg, B, K)
    mask, motion, _ = clip_constraint(cfg, B, K, cfg is not C.TINY)
    host = _clip(cfg, m, d, ins, "host", init, (mask, motion))
    assert not m.inpainting
    lib = _clip(cfg, m, d, ins, "library", init, (mask, motion))
    assert np.array_equal(host, lib) and not m.clip_init and not m.clip_inpainting
    lo = 3 if cfg is C.TINY else 0
    on = (mask != 0)[..., lo:]
    assert np.array_equal(lib[..., lo:][on], motion[..., lo:][on])
    assert not np.array_equal(lib, _clip(cfg, m, d, ins, "library", None, (mask, motion)))
    assert not np.array_equal(lib, _clip(cfg, m, d, ins, "library", init))


# ---- 8. lanes ---------------------------------------------------------------------------------------------------------------------------
def test_lanes(emu_lib):
    """two lanes x 2 clips, lane 0 with an init, lane 1 without: each lane bit-identical to the same lane run alone, lane 1 to a run with
    no init anywhere; the host form of the multi-lane drivers agrees"""
    for cfg in (C.TINY, C.TINY5):
        B, K, NL = 2, 3, 2
        m = _model(emu_lib, cfg, "bf16", B)
        lanes, d = [m, m.clone()], create_gaussian_diffusion(library=emu_lib)
        per = [_inputs(cfg, B, K, clip0=ln * B) for ln in range(NL)]
        feats = [p[0] for p in per]
        init = _init(cfg, B, K)

        def run(w, inits):
            kw = dict(seed=7, skip_timesteps=SKIP, stream_ids=[3, 4], kernel_set=None, windows=w, init_motion=inits)
            if cfg is C.TINY:
                return S.generate_clips_streams(lanes, d, feats, per[0][1], **kw)
            return S.generate_clips_streams_dsgplus(lanes, d, feats, per[0][1], [p[2] for p in per], K * cfg.stride, seed_lasts=[p[3] for p in per],
                                                    feature_division=1, **kw)
        lib = run("library", [init, None])
        assert lib.shape[0] == NL * B and np.array_equal(run("host", [init, None]), lib)
        free = run("library", None)
        assert np.array_equal(lib[B:], free[B:]) and not np.array_equal(lib[:B], free[:B])
        assert not lanes[0].clip_init and not lanes[1].clip_init
        for ln in range(NL):
            feats_l, style_l, seed_l, last_l = per[ln]
            kw = dict(seed=7, skip_timesteps=SKIP, stream_id=3 + ln, windows="library")
            if ln == 0:
                kw.update(init_motion=init)
            if cfg is C.TINY:
                alone = S.generate_clip(lanes[ln], d, feats_l, per[0][1], **kw)
            else:
                alone = S.generate_clip_dsgplus(lanes[ln], d, feats_l, per[0][1], seed_l, K * cfg.stride, seed_last=last_l, feature_division=1, **kw)
            assert np.array_equal(alone, lib[ln * B:(ln + 1) * B]), (cfg.name, ln)
        with pytest.raises(ValueError):
            run("library", [init])
        with pytest.raises(ValueError):
            run("host", [init])


# ---- 9. stickiness and refusals -----------------------------------------------------------------------------------------------------
def test_stickiness_and_refusals(emu_lib):
    cfg, B, K = C.TINY, 2, 2
    m, d = _model(emu_lib, cfg, "fp32", B + 1), create_gaussian_diffusion(library=emu_lib)
    ins = _inputs(cfg, B, K)
    feats, style, seed_pose, _ = ins
    init = _init(cfg, B, K)
    n_out = n_out_of(cfg, K, False)
    free = _clip(cfg, m, d, ins, "library")
    held = _clip(cfg, m, d, ins, "library", init)
    assert not np.array_equal(free, held)
    m.set_schedule(d)
    audio, sty, seed0 = L.Buf(np.stack(feats)), L.Buf(style), L.Buf(seed_pose)
    ones = L.Buf(np.ones((1, cfg.n_poses), np.uint8), "uint8")
    out = np.zeros((B, n_out, cfg.njoints), np.float32)

    def call(k=K, batch=B, o=out, init_image=None):
        a = L.dsg_sample_args()
        a.mode, a.skip_timesteps, a.seed, a.init_image = L.MODE_DDPM, SKIP, 5, init_image
        return emu_lib.cdll.dsg_sample_clip(m.handle, sty.p, seed0.p, audio.p, ones.p, 1, None, ctypes.byref(a), k, 1, 0, o.ctypes.data, batch, None)
    err = lambda: emu_lib.cdll.dsg_last_error().decode()
    # sticky: two calls in a row honour it
    m.set_clip_init(init, B)
    assert m.clip_init
    for _ in range(2):
        out[:] = 0
        assert call() == 0 and np.array_equal(out, held)
    # dsg_sample ignores it (and leaves it alone)
    y = synth_window_inputs(cfg, B, window=0, seed_pose_scale=0.3)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    one = d.manual_seed(9, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP)
    fresh = d.manual_seed(9, 1).p_sample_loop(_model(emu_lib, cfg, "fp32", B + 1), shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP)
    assert np.array_equal(one, fresh) and m.clip_init
    assert call() == 0 and np.array_equal(out, held)
    # n_frames != n_out (another K), another batch: DSG_E_INVALID with both numbers in the message
    big = np.zeros((B, n_out_of(cfg, K + 1, False), cfg.njoints), np.float32)
    assert call(k=K + 1, o=big) == -1 and str(n_out) in err() and str(big.shape[1]) in err() and "dsg_set_clip_init" in err()
    f8 = np.ascontiguousarray(np.stack([np.concatenate([f, f[:1]]) for f in feats]))      # (B + 1 clips of features)
    a3, s3, p3 = L.Buf(f8), L.Buf(np.concatenate([style, style[:1]])), L.Buf(np.concatenate([seed_pose, seed_pose[:1]]))
    o3 = np.zeros((B + 1, n_out, cfg.njoints), np.float32)
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps, a.seed = L.MODE_DDPM, SKIP, 5
    assert emu_lib.cdll.dsg_sample_clip(m.handle, s3.p, p3.p, a3.p, ones.p, 1, None, ctypes.byref(a), K, 1, 0, o3.ctypes.data, B + 1, None) == -1
    assert str(B) in err() and str(B + 1) in err() and "dsg_set_clip_init" in err()
    assert call() == 0 and np.array_equal(out, held)          # (a refused call leaves it as it was)
    # the setter through the bare ABI: B > max_batch, n_frames < 1
    f = emu_lib.cdll.dsg_set_clip_init
    vb = L.Buf(init)
    assert f(m.handle, vb.p, B + 2, n_out, None) == -1 and err()
    assert f(m.handle, vb.p, B, 0, None) == -1 and err()
    assert call() == 0 and np.array_equal(out, held)          # (refused settings left it alone too)
    # args.init_image is still refused, with or without a clip-level init
    wi = L.Buf(S.window_init(cfg, init, seed_pose, 0, False))
    assert call(init_image=wi.ptr) == -1 and "per window" in err()
    assert call() == 0 and np.array_equal(out, held)
    # a clone starts without one
    c = m.clone()
    assert c.clip_init is False
    assert np.array_equal(_clip(cfg, c, d, ins, "library"), free)
    # off (NULL): bit for bit the plain clip; a grown clip (more frames than before) replaces the copy
    m.set_clip_init(None, 0)
    assert not m.clip_init and call() == 0 and np.array_equal(out, free)
    assert call(init_image=wi.ptr) == -1 and "per window" in err()
    init3 = _init(cfg, B, K + 1)
    m.set_clip_init(init3, B)
    ins3 = _inputs(cfg, B, K + 1)
    a4 = L.Buf(np.stack(ins3[0]))
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps, a.seed = L.MODE_DDPM, SKIP, 5
    assert emu_lib.cdll.dsg_sample_clip(m.handle, sty.p, seed0.p, a4.p, ones.p, 1, None, ctypes.byref(a), K + 1, 1, 0, big.ctypes.data, B, None) == 0
    m.set_clip_init(None, 0)
    assert np.array_equal(big, _clip(cfg, m, d, ins3, "host", init3))
    # and back to the smaller one within the grown copy
    m.set_clip_init(init, B)
    assert call() == 0 and np.array_equal(out, held)
    m.set_clip_init(None, 0)
    # Python: a wrong shape; a custom sample_fn with windows="library"
    with pytest.raises(ValueError, match="shape"):
        _clip(cfg, m, d, ins, "library", init[:, :-1])
    with pytest.raises(ValueError):
        _clip(cfg, m, d, ins, "host", init[:, :-1])
    with pytest.raises(ValueError, match="shape"):
        m.set_clip_init(init[..., :-1], B)
    with pytest.raises(ValueError, match="shape"):
        d.sample_clip(m, feats, style, root_shift=True, keep_last_tail=False, skip_timesteps=SKIP, init_motion=init[:1])
    with pytest.raises(ValueError):
        S.generate_clip(m, d, feats, style, skip_timesteps=SKIP, sample_fn=d.p_sample_loop, windows="library", init_motion=init)
    assert not m.clip_init and np.array_equal(_clip(cfg, m, d, ins, "library"), free)


def test_skip_timesteps_zero_is_allowed(emu_lib):
    """skip_timesteps == 0: the reference noises the init to the LAST timestep (gaussian_diffusion.py:706-713) -- on a short schedule, so that
    the whole chain runs"""
    cfg, B, K = C.TINY, 2, 2
    m, d = _model(emu_lib, cfg, "bf16", B), create_gaussian_diffusion("4", library=emu_lib)
    ins = _inputs(cfg, B, K)
    init = _init(cfg, B, K)
    host = _clip(cfg, m, d, ins, "host", init, skip=0)
    lib = _clip(cfg, m, d, ins, "library", init, skip=0)
    assert np.array_equal(host, lib) and d._draw == K * (1 + d.num_timesteps)
    assert not np.array_equal(lib, _clip(cfg, m, d, ins, "library", skip=0))


# ---- 10. resource report --------------------------------------------------------------------------------------------------------------
def test_one_new_kernel_without_scratch(hip_lib_path):
    """the rebuilt code object: the start kernel is there once per instantiated precision policy (PF32, PBF16; bf16w2 handles take PBF16's),
    each with ScratchSize 0 (the register report is read as tests/test_emu_clip_inpaint.py reads it)"""
    import re
    from tests.test_emu_inpaint import _resource_report
    text = _resource_report()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch)
    new = sorted((n, s) for n, s in zip(names, scratch) if "k_clip_x_in" in n)
    assert len(new) == 2 and [s for _, s in new] == [0, 0]
    assert sum("PBF16E" in n for n, _ in new) == 1 and sum("PF32E" in n for n, _ in new) == 1
