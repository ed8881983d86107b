"""MI355X (-m gpu): editing an existing clip in one library call (dsg_set_clip_init, `init_motion` of the clip drivers): the start kernel
(k_clip_x_in: window cut + q_sample + state write) at the product widths -- J = 1141 / 2052 / 2232, where a clip row starts on every
4-byte phase -- bit for bit against the host window loop with `window_init(...)` as every window's `init_image` on the same handle under
the same kernel set; under every kernel set by name (the layout of the state shadow belongs to the set); DDIM; fused guidance; together
with the clip constraint; lanes; the oracle's inference() loop started from the same slices; and the kernel alone against a numpy
restatement of the stitch.  The emulator tests are tests/test_emu_clip_init.py."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.clip_init_util import clip_init, numpy_stitch
from tests.clip_inpaint_util import clip_constraint, n_out_of
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TOL_CHAIN_BF16 = 2e-2      # the bf16 chain bound of the GPU suite, as tests/test_gpu_clip.py:14
K, N_RUN = 3, 4
SKIP = 1000 - N_RUN


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


def _model(cfg, B, kset=None, prec="bf16"):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision=prec, max_batch=B, device=0)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    return m.set_kernel_set(kset) if kset else m


def _inputs(cfg, B, clip0=0, k=K):
    import torch
    ins = [synth_window_inputs(cfg, B, window=w, clip0=clip0, seed_pose_scale=0.2) for w in range(k)]
    return ins, [torch.from_numpy(y["audio"]).cuda() for y in ins]


def _zeggs(cfg):
    return cfg is C.ZEGGS


def _init(cfg, B, on_device=False, k=K):
    """the init motion [B, n_out, J] of tests/clip_init_util.py, as numpy and (on_device) as a tensor on the device"""
    init = clip_init(cfg, B, k, not _zeggs(cfg))
    if on_device:
        import torch
        return torch.from_numpy(init).cuda(), init
    return init, init


def _clip(cfg, m, d, ins, feats, windows, init=None, con=None, skip=SKIP, stream_id=0, ddim=False, eta=0.0):
    import torch
    from diffusestylegesture_amd.sample import generate_clip, generate_clip_dsgplus
    style = [1] + [0] * (cfg.style_dim_in - 1)
    kw = {} if init is None else dict(init_motion=init)
    if con is not None:
        kw.update(inpainting_mask=con[0], inpainted_motion=con[1])
    if _zeggs(cfg):
        return generate_clip(m, d, feats, style, seed=31, smoothing=True, skip_timesteps=skip, stream_id=stream_id, windows=windows, ddim=ddim,
                             eta=eta, **kw)
    return generate_clip_dsgplus(m, d, feats, style, torch.from_numpy(ins[0]["seed"]).cuda(), len(feats) * cfg.stride, seed=31, skip_timesteps=skip,
                                 stream_id=stream_id, feature_division=1, windows=windows, ddim=ddim, eta=eta, **kw)


@pytest.fixture(scope="module")
def zeggs_b3(gpu):
    """the ZEGGS clip of three clips edited from three init motions, library form, computed once: (model, diffusion, inputs, init, clip)"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 3
    m, d = _model(cfg, B), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    init_t, init = _init(cfg, B, on_device=True)
    lib = _clip(cfg, m, d, ins, feats, "library", init_t, stream_id=4)
    return m, d, ins, feats, init_t, init, lib


# ---- 1. bit identity, library against host loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,kset", [(C.ZEGGS, 3, None), (C.BEAT, 2, None), (C.TWH, 1, None), (C.ZEGGS, 16, "rows")],
                         ids=["zeggs-b3", "beat-b2", "twh-b1", "zeggs-b16-rows"])
def test_library_windows_bit_identical_to_host_loop(gpu, cfg, B, kset):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    m, d = _model(cfg, B, kset), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    init_in, init = _init(cfg, B, on_device=B == 2)
    host = _clip(cfg, m, d, ins, feats, "host", init_in)
    path, ks, draw = m.last_sample_path(), m.last_kernel_set(), d._draw
    lib = _clip(cfg, m, d, ins, feats, "library", init_in)
    assert host.shape == lib.shape == init.shape == (B, n_out_of(cfg, K, not _zeggs(cfg)), cfg.njoints)
    assert np.isfinite(lib).all() and np.array_equal(host, lib)
    assert m.last_sample_path() == path and m.last_kernel_set() == ks and (kset is None or ks == kset)
    assert d._draw == draw == K * (1 + N_RUN) and m.last_sample_ms()[1] == K * N_RUN
    assert not m.clip_init
    assert not np.array_equal(lib, _clip(cfg, m, d, ins, feats, "library"))


# ---- 2. the start kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B", [(C.ZEGGS, 2), (C.BEAT, 1)], ids=["zeggs", "beat"])
def test_start_kernel_alone_vs_numpy_stitch(gpu, cfg, B):
    """one step per window: the clip call is the start kernel, one pose head and the hand-off.  Yardstick: K p_sample_loop calls with
    init_image = window_init(...), stitched by the numpy restatement of tests/clip_init_util.py"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.sample import window_init
    m, d = _model(cfg, B), create_gaussian_diffusion()
    skip = d.num_timesteps - 1
    ins, feats = _inputs(cfg, B)
    zeggs = _zeggs(cfg)
    Sd, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
    _, init = _init(cfg, B)
    got = _clip(cfg, m, d, ins, feats, "library", init, skip=skip)
    d.manual_seed(31, 0)
    style = np.repeat(np.asarray([[1] + [0] * (cfg.style_dim_in - 1)], np.float32), B, 0)
    seed0 = None if zeggs else ins[0]["seed"]

    def sample_window(c, seed):
        y = {"style": style, "seed": seed, "audio": feats[c], "mask_local": np.ones((1, T), bool)}
        return d.p_sample_loop(m, (B, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip,
                               init_image=window_init(cfg, init, seed0, c, not zeggs)).cpu().numpy()
    want = numpy_stitch(zeggs, Sd, T, K, sample_window, np.zeros((B, J, 1, Sd), np.float32) if zeggs else seed0)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- 3. the state shadow's layout belongs to the kernel set -----------------------------------------------------------------------
@pytest.mark.parametrize("kset,prec", [("latency", "bf16"), ("tile", "bf16"), ("block", "bf16"), ("stream", "bf16"), ("rows", "bf16"),
                                       ("tile", "bf16w2"), ("tile", "fp32")],
                         ids=["latency", "tile", "block", "stream", "rows", "tile-bf16w2", "tile-fp32"])
def test_every_kernel_set_by_name(gpu, kset, prec):
    """ZEGGS, B = 3, K = 2, one step per window: the start kernel writes the shadow the named set's first GEMM reads"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B, k = C.ZEGGS, 3, 2
    m, d = _model(cfg, B, kset, prec), create_gaussian_diffusion()
    skip = d.num_timesteps - 1
    ins, feats = _inputs(cfg, B, k=k)
    _, init = _init(cfg, B, k=k)
    host = _clip(cfg, m, d, ins, feats, "host", init, skip=skip)
    assert m.last_kernel_set() == kset
    lib = _clip(cfg, m, d, ins, feats, "library", init, skip=skip)
    assert m.last_kernel_set() == kset and np.isfinite(lib).all() and np.array_equal(host, lib)


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------------------
def test_zeggs_clip_vs_oracle(zeggs_b3):
    """oracle.sampler.zeggs_clip, every window started from init_image = window_init(...), one clip of the three.
    Measured on the MI355X: rel-L2 8.6e-3 (bound 2e-2); the emulator's fp32 figures for the same construction are 4.1e-7 .. 1.3e-6,
    tests/test_emu_clip_init.py."""
    from diffusestylegesture_amd.sample import window_init
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    cfg, B, sid, b = C.ZEGGS, 3, 4, 1
    m, d, ins, feats, init_t, init, got = zeggs_b3
    ref, od = MDMOracle(synth_state_dict(cfg, 20240), cfg), OracleDiffusion()
    shape = (B, cfg.njoints, 1, cfg.n_poses)

    def sample_window(c, y):
        nf = lambda k: philox.normal_bj1t(shape, 31, c * (1 + N_RUN) + k, sid)[b:b + 1]
        return sampler.p_sample_loop(od, ref, (1,) + shape[1:], nf, {"y": y}, skip_timesteps=SKIP,
                                     init_image=window_init(cfg, init[b:b + 1], None, c, False))
    want = sampler.zeggs_clip(sample_window, cfg, [y["audio"][b:b + 1] for y in ins], [1, 0, 0, 0, 0, 0])
    e = rel_l2(got[b], want)
    print(f"library clip from an init motion (ZEGGS, K = {K}, {N_RUN} steps) vs oracle.sampler.zeggs_clip: rel-L2 {e:.3e}")
    assert e < TOL_CHAIN_BF16


# ---- 5. DDIM, 6. guidance -------------------------------------------------------------------------------------------------------------
def test_ddim(gpu):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 2
    m, d = _model(cfg, B), create_gaussian_diffusion("ddim50")
    ins, feats = _inputs(cfg, B)
    _, init = _init(cfg, B)
    skip = d.num_timesteps - N_RUN
    host = _clip(cfg, m, d, ins, feats, "host", init, skip=skip, ddim=True, eta=1.0)
    draw = d._draw
    lib = _clip(cfg, m, d, ins, feats, "library", init, skip=skip, ddim=True, eta=1.0)
    assert np.array_equal(host, lib) and d._draw == draw == K * (1 + N_RUN)


@pytest.mark.parametrize("cfg,kset", [(C.ZEGGS, None), (C.BEATPP, "rows")], ids=["zeggs", "beatpp-rows"])
def test_guided(gpu, cfg, kset):
    """fused classifier-free guidance (twins in the batch, max_batch = 2 B): the host loop written out with y['scale'] and the window's
    init_image against sample_clip; the twins must receive the same start"""
    import torch
    from diffusestylegesture_amd import sample as S
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    B = 2
    zeggs = _zeggs(cfg)
    m, d = ClassifierFreeSampleModel(_model(cfg, 2 * B, kset)), create_gaussian_diffusion()
    Sd, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
    y0 = synth_window_inputs(cfg, B, window=0, seed_pose_scale=0.2)
    src = cfg if zeggs else C.BEAT             # (features as the DSG+ drivers take them: they cut the closing S frames of DiffuseStyleGesture++ themselves)
    feats = [torch.from_numpy(synth_window_inputs(src, B, window=w)["audio"]).cuda() for w in range(K)]
    style = torch.from_numpy(y0["style"]).cuda()
    seed0 = torch.from_numpy(y0["seed"]).cuda()
    seed_last = None if zeggs else torch.from_numpy(y0["seed_last"]).cuda()
    init_t, _ = _init(cfg, B, on_device=True)
    scale = torch.tensor([2.5, 0.5]).cuda()
    ones = torch.ones(1, T, dtype=torch.bool).cuda()
    out = []
    d.manual_seed(11, 3)
    for c in range(K):
        if zeggs:
            y = S._zeggs_window_y(cfg, feats[c], style, out[-1] if out else None, seed0, True, ones)
        else:
            y = S._dsgplus_window_y(cfg, feats, c, style, seed0 if c == 0 else out[-1][..., -Sd:], seed_last, True, ones)
        s = d.p_sample_loop(m, (B, J, 1, T), clip_denoised=False, skip_timesteps=SKIP, model_kwargs={"y": dict(y, scale=scale)},
                            init_image=S.window_init(cfg, init_t, seed0, c, not zeggs))
        if zeggs:
            S._zeggs_stitch(out, s, Sd, True, True)
        else:
            S._dsgplus_stitch(out, s, Sd, True)
    host = S._zeggs_finish(out, Sd, True) if zeggs else S._dsgplus_finish(out, Sd, J, K * cfg.stride, 1, True)
    ks, draw = m.model.last_kernel_set(), d._draw
    audio = feats if zeggs else [S._dsgplus_window_y(cfg, feats, c, style, seed0, seed_last, True, None)["audio"] for c in range(K)]
    lib = d.manual_seed(11, 3).sample_clip(m, audio, style, seed0=seed0, root_shift=zeggs, keep_last_tail=not zeggs, skip_timesteps=SKIP,
                                           scale=scale, seed_last=seed_last, init_motion=init_t)
    assert np.array_equal(host, lib) and d._draw == draw and m.model.last_kernel_set() == ks and (kset is None or ks == kset)


# ---- 7. with the clip constraint ------------------------------------------------------------------------------------------------------
def test_with_clip_constraint(gpu):
    """init and constraint together: bit identity, and the constraint holds exactly (features >= 3: the root shift moves the root channels)"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 3
    m, d = _model(cfg, B), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    _, init = _init(cfg, B)
    mask, motion, _ = clip_constraint(cfg, B, K, False)
    host = _clip(cfg, m, d, ins, feats, "host", init, (mask, motion))
    lib = _clip(cfg, m, d, ins, feats, "library", init, (mask, motion))
    assert np.array_equal(host, lib) and not m.clip_init and not m.clip_inpainting and not m.inpainting
    on = (mask != 0)[..., 3:]
    assert np.array_equal(lib[..., 3:][on], motion[..., 3:][on])
    assert not np.array_equal(lib, _clip(cfg, m, d, ins, feats, "library", None, (mask, motion)))


# ---- 8. lanes ---------------------------------------------------------------------------------------------------------------------------
def test_lanes(gpu):
    """2 lanes x 2 clips, lane 0 with an init, lane 1 without: each lane bit-identical to the same lane run alone, lane 1 to a run with no
    init anywhere"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.sample import generate_clip, generate_clips_streams
    cfg, NL, B = C.ZEGGS, 2, 2
    m = _model(cfg, B)
    lanes, d = [m, m.clone()], create_gaussian_diffusion()
    feats = [_inputs(cfg, B, clip0=ln * B)[1] for ln in range(NL)]
    _, init = _init(cfg, B)
    style = [0, 1, 0, 0, 0, 0]
    run = lambda inits: generate_clips_streams(lanes, d, feats, style, seed=17, skip_timesteps=SKIP, stream_ids=[5, 6], kernel_set=None,
                                               windows="library", init_motion=inits)
    lib = run([init, None])
    free = run(None)
    assert np.array_equal(lib[B:], free[B:]) and not np.array_equal(lib[:B], free[:B])
    for ln in range(NL):
        kw = {} if ln else dict(init_motion=init)
        alone = generate_clip(lanes[ln], d, feats[ln], style, seed=17, skip_timesteps=SKIP, stream_id=5 + ln, windows="library", **kw)
        assert np.array_equal(alone, lib[ln * B:(ln + 1) * B]), ln


# ---- 9. stickiness --------------------------------------------------------------------------------------------------------------------
def test_stickiness(zeggs_b3):
    """the single-window loop ignores a clip-level init; after set_clip_init(None, 0) the clip is the plain one; a clone starts without one"""
    import torch
    cfg, B = C.ZEGGS, 3
    m, d, ins, feats, init_t, init, held = zeggs_b3
    free = _clip(cfg, m, d, ins, feats, "library", stream_id=4)
    assert not np.array_equal(free, held)
    y = {k: torch.from_numpy(v).cuda() for k, v in ins[0].items()}
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    one = d.manual_seed(9, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP).cpu().numpy()
    m.set_clip_init(init_t, B)
    assert m.clip_init and m.clone().clip_init is False
    two = d.manual_seed(9, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP).cpu().numpy()
    assert np.array_equal(one, two) and m.clip_init
    m.set_clip_init(None, 0)
    assert not m.clip_init and np.array_equal(_clip(cfg, m, d, ins, feats, "library", stream_id=4), free)
