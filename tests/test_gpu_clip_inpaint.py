"""MI355X (-m gpu): motion inpainting over a whole clip (dsg_set_clip_inpainting, `inpainting_mask` / `inpainted_motion` of the clip drivers): the
cut kernel (k_clip_inp_window) at the product widths -- J = 1141 / 2052 / 2232, where a clip row starts on every 4-byte phase and a quad's
mask bytes on every byte phase -- bit for bit against the host window loop with `window_constraint(...)` in y on the same handle under the
same kernel set; exactly where the mask is set; DDIM; fused guidance; lanes; the oracle's inference() loop with the constraint as its
denoised_fn; and the kernel alone against a numpy restatement of the stitch.  The emulator tests are tests/test_emu_clip_inpaint.py."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
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


def _model(cfg, B, kset=None):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision="bf16", max_batch=B, device=0)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    return m.set_kernel_set(kset) if kset else m


def _inputs(cfg, B, clip0=0):
    import torch
    ins = [synth_window_inputs(cfg, B, window=w, clip0=clip0, seed_pose_scale=0.2) for w in range(K)]
    return ins, [torch.from_numpy(y["audio"]).cuda() for y in ins]


def _zeggs(cfg):
    return cfg is C.ZEGGS


def _con(cfg, B, first=0, on_device=False):
    """(mask, motion) [B, n_out, J] of tests/clip_inpaint_util.py, as numpy or as tensors on the device"""
    mask, motion, kinds = clip_constraint(cfg, B, K, not _zeggs(cfg), first=first)
    if on_device:
        import torch
        return (torch.from_numpy(mask).cuda(), torch.from_numpy(motion).cuda()), (mask, motion), kinds
    return (mask, motion), (mask, motion), kinds


def _clip(cfg, m, d, ins, feats, windows, con=None, skip=SKIP, stream_id=0, ddim=False, eta=0.0):
    import torch
    from diffusestylegesture_amd.sample import generate_clip, generate_clip_dsgplus
    style = [1] + [0] * (cfg.style_dim_in - 1)
    kw = {} if con is None else dict(inpainting_mask=con[0], inpainted_motion=con[1])
    if _zeggs(cfg):
        return generate_clip(m, d, feats, style, seed=31, smoothing=True, skip_timesteps=skip, stream_id=stream_id, windows=windows, ddim=ddim,
                             eta=eta, **kw)
    return generate_clip_dsgplus(m, d, feats, style, torch.from_numpy(ins[0]["seed"]).cuda(), K * cfg.stride, seed=31, skip_timesteps=skip,
                                 stream_id=stream_id, feature_division=1, windows=windows, ddim=ddim, eta=eta, **kw)


def _holds(cfg, out, mask, motion, kinds, root_shift):
    """DDPM / DDIM without the clamp: the last step returns x0, the blend of two equal values the value.  With the root shift: features >= 3; all
    features of the clip whose mask holds the hand-off frames (the shift delta of a constrained root channel is 0 there)"""
    on = mask != 0
    if not root_shift:
        return np.array_equal(out[on], motion[on])
    ok = np.array_equal(out[..., 3:][on[..., 3:]], motion[..., 3:][on[..., 3:]])
    for b, kind in enumerate(kinds):
        if kind == "frames":
            ok = ok and on[b, :, :3].any() and np.array_equal(out[b][on[b]], motion[b][on[b]])
    return ok


@pytest.fixture(scope="module")
def zeggs_b3(gpu):
    """the ZEGGS clip of three differently masked clips, library form, computed once: (model, inputs, constraint, kinds, clip)"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 3
    m, d = _model(cfg, B), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    con, (mask, motion), kinds = _con(cfg, B, on_device=True)
    lib = _clip(cfg, m, d, ins, feats, "library", con, stream_id=4)
    return m, d, ins, feats, con, mask, motion, kinds, lib


# ---- 1. + 2. bit identity, library against host loop; the constraint holds exactly -----------------------------------------------------
@pytest.mark.parametrize("cfg,B,kset", [(C.ZEGGS, 3, None), (C.BEAT, 2, None), (C.TWH, 1, None), (C.ZEGGS, 16, "rows")],
                         ids=["zeggs-b3", "beat-b2", "twh-b1", "zeggs-b16-rows"])
def test_library_windows_bit_identical_to_host_loop(gpu, cfg, B, kset):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    m, d = _model(cfg, B, kset), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    con, (mask, motion), kinds = _con(cfg, B, first=2 if B == 1 else 0, on_device=B == 2)      # (B = 1: the checkerboard)
    host = _clip(cfg, m, d, ins, feats, "host", con)
    path, ks, draw = m.last_sample_path(), m.last_kernel_set(), d._draw
    lib = _clip(cfg, m, d, ins, feats, "library", con)
    assert host.shape == lib.shape == mask.shape == (B, n_out_of(cfg, K, not _zeggs(cfg)), cfg.njoints)
    assert np.isfinite(lib).all() and np.array_equal(host, lib)
    assert m.last_sample_path() == path and m.last_kernel_set() == ks and (kset is None or ks == kset)
    assert d._draw == draw == K * (1 + N_RUN) and m.last_sample_ms()[1] == K * N_RUN
    assert not m.clip_inpainting and not m.inpainting
    assert _holds(cfg, lib, mask, motion, kinds, _zeggs(cfg))
    assert not np.array_equal(lib[mask == 0], motion[mask == 0])


def test_constraint_then_clamp_without_root_shift(gpu):
    """root_shift = 0, clip_denoised=True: every masked element, root channels included, is np.clip(motion, -1, 1)"""
    import torch
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 3
    m, d = _model(cfg, B), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    con, (mask, motion), _ = _con(cfg, B)
    style = torch.tensor([[1.0] + [0.0] * (cfg.style_dim_in - 1)] * B).cuda()
    out = d.manual_seed(31, 0).sample_clip(m, feats, style, root_shift=False, keep_last_tail=False, skip_timesteps=SKIP, clip_denoised=True,
                                           inpainting_mask=con[0], inpainted_motion=con[1])
    on = mask != 0
    assert (np.abs(motion[on]) > 1).any() and np.array_equal(out[on], np.clip(motion, -1, 1)[on])


# ---- 3. the cut kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B", [(C.ZEGGS, 2), (C.BEAT, 1)], ids=["zeggs", "beat"])
def test_cut_kernel_alone_vs_numpy_stitch(gpu, cfg, B):
    """one step per window: the clip call is the cut kernel, one pose head and the hand-off.  Yardstick: K p_sample_loop calls with
    y['inpainting_*'] = window_constraint(...), stitched by the numpy restatement of tests/test_gpu_clip.py:105-133"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.sample import window_constraint
    m, d = _model(cfg, B), create_gaussian_diffusion()
    skip = d.num_timesteps - 1
    ins, feats = _inputs(cfg, B)
    zeggs = _zeggs(cfg)
    Sd, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
    con, (mask, motion), _ = _con(cfg, B, first=1)
    got = _clip(cfg, m, d, ins, feats, "library", con, skip=skip)
    d.manual_seed(31, 0)
    style = np.repeat(np.asarray([[1] + [0] * (cfg.style_dim_in - 1)], np.float32), B, 0)
    tail = np.zeros((B, J, 1, Sd), np.float32) if zeggs else ins[0]["seed"]
    rows = []                                  # frame-major pieces [B, frames, J]
    for c in range(K):
        wm, wv = window_constraint(cfg, mask, motion, c, not zeggs)
        y = {"style": style, "seed": np.ascontiguousarray(tail), "audio": feats[c], "mask_local": np.ones((1, T), bool),
             "inpainting_mask": wm, "inpainted_motion": wv}
        s = d.p_sample_loop(m, (B, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip).cpu().numpy()[:, :, 0, :]
        s = s.transpose(0, 2, 1).copy()        # [B, T, J]
        if c > 0:
            last0 = tail[:, :, 0, 0]           # frame 0 of the previous window's tail, [B, J]
            if zeggs:
                delta = s[:, 0, :3] - last0[:, :3]
                s[:, :, :3] = s[:, :, :3] - delta[:, None, :]
            s[:, 0] = last0 * np.float32(0.5) + s[:, 0] * np.float32(0.5)
        tail = s[:, T - Sd:].transpose(0, 2, 1)[:, :, None, :]
        rows.append(s if (c == K - 1 and not zeggs) else s[:, : T - Sd])
    want = np.concatenate(rows, 1)[:, Sd:]
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------------------
def test_zeggs_clip_vs_oracle(zeggs_b3):
    """oracle.sampler.zeggs_clip with denoised_fn = the window's constraint (tests/test_inpaint_golden.py: inpaint_fn), rel-L2 over the
    unmasked elements of the clip whose mask holds whole frames at every boundary of the cut.  (Not measured on hardware yet; the emulator's
    fp32 figures for the same construction are 3.2e-7 .. 1.1e-6, tests/test_emu_clip_inpaint.py.)"""
    from diffusestylegesture_amd.sample import window_constraint
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    from tests.test_inpaint_golden import inpaint_fn
    cfg, B, sid = C.ZEGGS, 3, 4
    m, d, ins, feats, con, mask, motion, kinds, got = zeggs_b3
    b = kinds.index("frames")
    ref, od = MDMOracle(synth_state_dict(cfg, 20240), cfg), OracleDiffusion()
    shape = (B, cfg.njoints, 1, cfg.n_poses)

    def sample_window(c, y):
        nf = lambda k: philox.normal_bj1t(shape, 31, c * (1 + N_RUN) + k, sid)[b:b + 1]
        wm, wv = window_constraint(cfg, mask[b:b + 1], motion[b:b + 1], c, False)
        return sampler.p_sample_loop(od, ref, (1,) + shape[1:], nf, {"y": y}, skip_timesteps=SKIP, denoised_fn=inpaint_fn(wm, wv))
    want = sampler.zeggs_clip(sample_window, cfg, [y["audio"][b:b + 1] for y in ins], [1, 0, 0, 0, 0, 0])
    free = mask[b] == 0
    e = rel_l2(got[b][free], want[free])
    print(f"constrained library clip (ZEGGS, K = {K}, {N_RUN} steps, mask 'frames') vs oracle.sampler.zeggs_clip, unmasked elements: rel-L2 {e:.3e}")
    assert 2 * np.count_nonzero(free) >= free.size and e < TOL_CHAIN_BF16
    assert np.array_equal(got[b][~free], want[~free])          # (the masked elements: the motion itself on both sides)


# ---- 5. DDIM and guidance -----------------------------------------------------------------------------------------------------------
def test_ddim(gpu):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 2
    m, d = _model(cfg, B), create_gaussian_diffusion("ddim50")
    ins, feats = _inputs(cfg, B)
    con, (mask, motion), kinds = _con(cfg, B, first=1)
    skip = d.num_timesteps - N_RUN
    host = _clip(cfg, m, d, ins, feats, "host", con, skip=skip, ddim=True, eta=1.0)
    draw = d._draw
    lib = _clip(cfg, m, d, ins, feats, "library", con, skip=skip, ddim=True, eta=1.0)
    assert np.array_equal(host, lib) and d._draw == draw == K * (1 + N_RUN)
    assert _holds(cfg, lib, mask, motion, kinds, True)


@pytest.mark.parametrize("cfg,kset", [(C.ZEGGS, None), (C.BEATPP, "rows")], ids=["zeggs", "beatpp-rows"])
def test_guided(gpu, cfg, kset):
    """fused classifier-free guidance (twins in the batch, max_batch = 2 B): the host loop written out with y['scale'] and the window's
    constraint against sample_clip; the constraint acts on the combined prediction, so it holds exactly"""
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
    con, (mask, motion), kinds = _con(cfg, B, first=1, on_device=True)
    scale = torch.tensor([2.5, 0.5]).cuda()
    ones = torch.ones(1, T, dtype=torch.bool).cuda()
    out = []
    d.manual_seed(11, 3)
    for c in range(K):
        if zeggs:
            y = S._zeggs_window_y(cfg, feats[c], style, out[-1] if out else None, seed0, True, ones)
        else:
            y = S._dsgplus_window_y(cfg, feats, c, style, seed0 if c == 0 else out[-1][..., -Sd:], seed_last, True, ones)
        wm, wv = S.window_constraint(cfg, con[0], con[1], c, not zeggs)
        s = d.p_sample_loop(m, (B, J, 1, T), clip_denoised=False, skip_timesteps=SKIP,
                            model_kwargs={"y": dict(y, scale=scale, inpainting_mask=wm, inpainted_motion=wv)})
        if zeggs:
            S._zeggs_stitch(out, s, Sd, True, True)
        else:
            S._dsgplus_stitch(out, s, Sd, True)
    host = S._zeggs_finish(out, Sd, True) if zeggs else S._dsgplus_finish(out, Sd, J, K * cfg.stride, 1, True)
    ks, draw = m.model.last_kernel_set(), d._draw
    m.model.set_inpainting(None, None, 0)
    audio = feats if zeggs else [S._dsgplus_window_y(cfg, feats, c, style, seed0, seed_last, True, None)["audio"] for c in range(K)]
    lib = d.manual_seed(11, 3).sample_clip(m, audio, style, seed0=seed0, root_shift=zeggs, keep_last_tail=not zeggs, skip_timesteps=SKIP,
                                           scale=scale, seed_last=seed_last, inpainting_mask=con[0], inpainted_motion=con[1])
    assert np.array_equal(host, lib) and d._draw == draw and m.model.last_kernel_set() == ks and (kset is None or ks == kset)
    assert _holds(cfg, lib, mask, motion, kinds, zeggs)


# ---- 6. lanes ---------------------------------------------------------------------------------------------------------------------------
def test_lanes(gpu):
    """2 lanes x 2 clips, lane 0 constrained, lane 1 not: each lane bit-identical to the same lane run alone, lane 1 to a run with no
    constraint anywhere"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.sample import generate_clip, generate_clips_streams
    cfg, NL, B = C.ZEGGS, 2, 2
    m = _model(cfg, B)
    lanes, d = [m, m.clone()], create_gaussian_diffusion()
    feats = [_inputs(cfg, B, clip0=ln * B)[1] for ln in range(NL)]
    con, (mask, motion), kinds = _con(cfg, B, first=1)
    style = [0, 1, 0, 0, 0, 0]
    run = lambda masks, motions: generate_clips_streams(lanes, d, feats, style, seed=17, skip_timesteps=SKIP, stream_ids=[5, 6], kernel_set=None,
                                                        windows="library", inpainting_mask=masks, inpainted_motion=motions)
    lib = run([con[0], None], [con[1], None])
    free = run(None, None)
    assert np.array_equal(lib[B:], free[B:]) and not np.array_equal(lib[:B], free[:B])
    assert _holds(cfg, lib[:B], mask, motion, kinds, True)
    for ln in range(NL):
        kw = {} if ln else dict(inpainting_mask=con[0], inpainted_motion=con[1])
        alone = generate_clip(lanes[ln], d, feats[ln], style, seed=17, skip_timesteps=SKIP, stream_id=5 + ln, windows="library", **kw)
        assert np.array_equal(alone, lib[ln * B:(ln + 1) * B]), ln


# ---- 7. stickiness --------------------------------------------------------------------------------------------------------------------
def test_stickiness(zeggs_b3):
    """the single-window loop ignores a clip-level constraint; after set_clip_inpainting(None, None, 0) the clip is the unconstrained one;
    a clone starts without one"""
    import torch
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, B = C.ZEGGS, 3
    m, d, ins, feats, con, mask, motion, kinds, held = zeggs_b3
    free = _clip(cfg, m, d, ins, feats, "library", stream_id=4)
    assert not np.array_equal(free, held)
    y = {k: torch.from_numpy(v).cuda() for k, v in ins[0].items()}
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    one = d.manual_seed(9, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP).cpu().numpy()
    m.set_clip_inpainting(con[0], con[1], B)
    assert m.clip_inpainting and m.clone().clip_inpainting is False
    two = d.manual_seed(9, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP).cpu().numpy()
    assert np.array_equal(one, two) and m.clip_inpainting
    m.set_clip_inpainting(None, None, 0)
    assert not m.clip_inpainting and np.array_equal(_clip(cfg, m, d, ins, feats, "library", stream_id=4), free)
