"""GPU: motion inpainting in the fused sampling loop (y['inpainting_mask'] / y['inpainted_motion'], gaussian_diffusion.py:317-321), through the
C ABI.  Every test here fails without the feature: the keys used to be ignored.

Yardsticks: the reference's own loops at the tiny dims (G18), and at the full dims the CPU oracle driven with
`denoised_fn = where(mask, motion, x0)`, which tests/test_inpaint_golden.py pins against G18.

Unmasked elements, rel-L2 against the oracle (MEASURED on MI355X, see MEASURED below); masked elements: bit-exact.  The last step of a chain
has posterior_mean_coef1 == 1, coef2 == 0 and adds no noise (DDPM), alphas_cumprod_prev[0] == 1 (DDIM: k3 = 1, k4 = k5 = 0), so with
clip_denoised off the final sample IS the motion wherever the mask is set -- derived, not measured."""
import os

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.test_inpaint_golden import inpaint_fn
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TOL_G18_FP32 = 1e-4          # the bound of the G17 hook test (test_gpu_round5.py)
# unmasked elements against the oracle: rel-L2 MEASURED on MI355X, per case and compared row; each case is asserted at twice its own value
# (the project's convention, DESIGN s2), never above the bound of the unconstrained chains (fp32 1e-4, bf16 2e-2, bf16w2 1.5e-3).
# (G18, fp32: 4.3e-7 .. 5.1e-7 against the reference's loops; generic loop against the fused one 3.0e-7.)
CAP_UNCONSTRAINED = {"bf16": 2e-2, "bf16w2": 1.5e-3}
MEASURED = {      # (set, sampler) -> rel-L2 of rows 0, 1; 40-step DDPM / DDIM-50 at the ZEGGS dims
    ("latency", "ddpm"): (1.04e-2,), ("latency", "ddim"): (8.8e-3,),                          # bf16, batch 1
    ("rows", "ddpm"): (9.9e-3, 8.2e-3), ("rows", "ddim"): (8.8e-3, 7.4e-3),                   # bf16, batch 16
    ("stream", "ddpm"): (1.02e-2, 8.4e-3), ("stream", "ddim"): (9.4e-3, 7.2e-3),              # bf16, batch 48
    ("tile", "ddpm"): (6.5e-4, 6.1e-4), ("tile", "ddim"): (5.9e-4, 4.6e-4),                   # bf16w2, batch 4
    ("beat-guided", "ddpm"): (6.8e-3, 1.08e-2),                                               # bf16, batch 8, 12 steps, rows 0 and 7
}


def _bound(prec, case, sampler_name, k):
    """twice the value measured for this case and row; BEAT row 7 (2 x 1.08e-2) is held at the unconstrained 2e-2"""
    return min(2 * MEASURED[case, sampler_name][k], CAP_UNCONSTRAINED[prec])


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


def _model(cfg, prec, max_batch=1, wseed=20240, **kw):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision=prec, max_batch=max_batch, device=0, **kw)
    m.load_state_dict(synth_state_dict(cfg, wseed))
    return m


def _y(y, mask, motion):
    return {"y": dict(y, inpainting_mask=mask, inpainted_motion=motion)}


def _edit_mask(cfg, B):
    """root and lower-body columns (the first third of the feature vector) for all frames, plus all columns of frames 0..15 for odd elements"""
    mask = np.zeros((B, cfg.njoints, 1, cfg.n_poses), bool)
    mask[:, :cfg.njoints // 3] = True
    mask[1::2, :, :, 0:16] = True
    return mask


def _motion(cfg, B, seed=1818):
    return np.stack([(0.8 * np.random.RandomState(seed + b).randn(cfg.njoints, 1, cfg.n_poses)).astype(np.float32) for b in range(B)])


def _rows(y, b):
    return {k: (v[b:b + 1] if k != "mask_local" else v) for k, v in y.items()}


def test_g18_fp32_fused_generic_and_progressive(gpu, golden_dir):
    """the reference's own loops at the tiny dims in fp32: fused DDPM (with / without the clamp) and DDIM; the generic loop (a plain callable
    around the denoiser) equals the fused loop within the fp32 chain bound of the emulator tests; with denoised_fn the constraint comes first;
    the progressive form is the one-call loop bit for bit"""
    import torch
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    g = np.load(os.path.join(golden_dir, "g18_inpaint_tiny.npz"))
    cfg, B = C.TINY, 2
    m = _model(cfg, "fp32", max_batch=B, wseed=int(g["wseed"]))
    shape, seed, motion = (B, cfg.njoints, 1, cfg.n_poses), int(g["noise_seed"]), g["motion"]
    y = synth_window_inputs(cfg, B, window=2, seed_pose_scale=0.3)
    d, d50 = create_gaussian_diffusion(), create_gaussian_diffusion("ddim50")
    mask = g["mask_joints"]
    s = np.asarray(d.manual_seed(seed, 21).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), skip_timesteps=800))
    print("G18 ddpm joints", rel_l2(s, g["ddpm_joints_skip800"]))
    assert rel_l2(s, g["ddpm_joints_skip800"]) < TOL_G18_FP32 and np.array_equal(s[mask], motion[mask])
    assert m.last_sample_path() == "aql" and m.last_sample_fence_free()
    mask = g["mask_frames"]
    s = np.asarray(d.manual_seed(seed, 22).p_sample_loop(m, shape, clip_denoised=True, model_kwargs=_y(y, mask, motion), skip_timesteps=800))
    print("G18 ddpm frames clip", rel_l2(s, g["ddpm_frames_clip_skip800"]))
    assert rel_l2(s, g["ddpm_frames_clip_skip800"]) < TOL_G18_FP32 and np.array_equal(s[mask], np.clip(motion, -1, 1)[mask])
    mask = g["mask_checker"]
    s = np.asarray(d50.manual_seed(seed, 23).ddim_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), eta=0.5))
    print("G18 ddim50 checker", rel_l2(s, g["ddim50_checker_eta05"]))
    assert rel_l2(s, g["ddim50_checker_eta05"]) < TOL_G18_FP32 and np.array_equal(s[mask], motion[mask])
    # torch inputs on the device; the generic loop: a plain callable, and a denoised_fn (applied AFTER the constraint)
    mask = g["mask_joints"]
    yt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in _y(y, mask, motion)["y"].items()}

    class Plain:
        def parameters(self):
            return m.parameters()

        def __call__(self, x, t, y=None):
            return m(x, t, y)
    fused = d.manual_seed(seed, 21).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": yt}, skip_timesteps=800).cpu().numpy()
    assert np.array_equal(fused, np.asarray(d.manual_seed(seed, 21).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion),
                                                                                  skip_timesteps=800)))
    gen = d.manual_seed(seed, 21).p_sample_loop(Plain(), shape, clip_denoised=False, model_kwargs={"y": yt}, skip_timesteps=800).cpu().numpy()
    print("generic vs fused", rel_l2(gen, fused))
    assert rel_l2(gen, fused) < 3e-5 and np.array_equal(gen[mask], motion[mask])
    s = d.manual_seed(seed, 24).p_sample_loop(m, shape, clip_denoised=False, denoised_fn=lambda x: 0.9 * x + 0.01, model_kwargs={"y": yt},
                                              skip_timesteps=800).cpu().numpy()
    print("G18 ddpm joints + hook", rel_l2(s, g["ddpm_joints_hook_skip800"]))
    assert rel_l2(s, g["ddpm_joints_hook_skip800"]) < TOL_G18_FP32
    outs = [o["sample"] for o in d.manual_seed(seed, 21).p_sample_loop_progressive(m, shape, clip_denoised=False, model_kwargs={"y": yt},
                                                                                   skip_timesteps=800)]
    assert len(outs) == 200 and np.array_equal(outs[-1].cpu().numpy(), fused)
    # without the keys the lane is back to the unconstrained chain
    plain = np.asarray(d.manual_seed(seed, 21).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=800))
    fresh = np.asarray(d.manual_seed(seed, 21).p_sample_loop(_model(cfg, "fp32", max_batch=B, wseed=int(g["wseed"])), shape, clip_denoised=False,
                                                             model_kwargs={"y": y}, skip_timesteps=800))
    assert np.array_equal(plain, fresh) and rel_l2(plain, fused) > 1e-2
    # the generic loop checks the shapes of both keys before it does anything
    for bad in (dict(yt, inpainting_mask=yt["inpainting_mask"][:, :-1]), dict(yt, inpainted_motion=yt["inpainted_motion"][..., :-1])):
        with pytest.raises(ValueError, match=r"y\['inpaint\w+'\] shape"):
            d.manual_seed(seed, 21).p_sample_loop(Plain(), shape, clip_denoised=False, model_kwargs={"y": bad}, skip_timesteps=998)


def test_const_noise_shares_the_noise_not_the_constraint(gpu, golden_dir):
    """const_noise gives every batch element the step noise of element 0; each element keeps its own mask and motion.  Tiny dims, fp32, the fused
    loop and the generic loop (a plain callable) against the oracle's const_noise loop driven with the constraint as its denoised_fn, at the
    fp32 chain bound (1e-4; rounding alone separates them, as for G18: measured 5.5e-7 fused, 5.5e-7 generic)."""
    import torch
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from oracle import sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    g = np.load(os.path.join(golden_dir, "g18_inpaint_tiny.npz"))
    cfg, B = C.TINY, 2
    m = _model(cfg, "fp32", max_batch=B, wseed=int(g["wseed"]))
    shape, motion, mask = (B, cfg.njoints, 1, cfg.n_poses), g["motion"], g["mask_frames"]      # frames 0..5 of element 0, 9..16 of element 1
    y = synth_window_inputs(cfg, B, window=2, seed_pose_scale=0.3)
    d = create_gaussian_diffusion()
    want = sampler.p_sample_loop(OracleDiffusion(), MDMOracle(synth_state_dict(cfg, int(g["wseed"])), cfg), shape, sampler.philox_noise_fn(shape, 77, 5),
                                 {"y": y}, skip_timesteps=994, const_noise=True, denoised_fn=inpaint_fn(mask, motion))
    s = np.asarray(d.manual_seed(77, 5).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), skip_timesteps=994, const_noise=True))
    print("const_noise + constraint, fused", rel_l2(s, want))
    assert rel_l2(s, want) < TOL_G18_FP32 and np.array_equal(s[mask], motion[mask])

    class Plain:
        def parameters(self):
            return m.parameters()

        def __call__(self, x, t, y=None):
            return m(x, t, y)
    yt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in _y(y, mask, motion)["y"].items()}
    gen = d.manual_seed(77, 5).p_sample_loop(Plain(), shape, clip_denoised=False, model_kwargs={"y": yt}, skip_timesteps=994, const_noise=True).cpu().numpy()
    print("const_noise + constraint, generic", rel_l2(gen, want))
    assert rel_l2(gen, want) < TOL_G18_FP32 and np.array_equal(gen[mask], motion[mask])


_ORACLE = {}


def _zeggs_oracle(sampler_name, b, y48, mask48, motion48):
    """row b of the ZEGGS case (rows do not interact: the oracle runs it as a batch of one), cached across the kernel sets"""
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    key = (sampler_name, b)
    if key not in _ORACLE:
        cfg = C.ZEGGS
        if "model" not in _ORACLE:
            _ORACLE["model"] = MDMOracle(synth_state_dict(cfg, 20240), cfg)
        shape = (48, cfg.njoints, 1, cfg.n_poses)
        fn = inpaint_fn(mask48[b:b + 1], motion48[b:b + 1])
        if sampler_name == "ddpm":
            _ORACLE[key] = sampler.p_sample_loop(OracleDiffusion(), _ORACLE["model"], (1,) + shape[1:], lambda k: philox.normal_bj1t(shape, 31, k, 7)[b:b + 1],
                                                 {"y": _rows(y48, b)}, skip_timesteps=960, denoised_fn=fn)
        else:
            _ORACLE[key] = sampler.ddim_sample_loop(OracleDiffusion(timestep_respacing="ddim50"), _ORACLE["model"], (1,) + shape[1:],
                                                    lambda k: philox.normal_bj1t(shape, 31, k, 8)[b:b + 1], {"y": _rows(y48, b)}, eta=0.5, denoised_fn=fn)
    return _ORACLE[key]


@pytest.mark.parametrize("prec,kset,B", [("bf16", "latency", 1), ("bf16", "rows", 16), ("bf16", "stream", 48), ("bf16w2", "tile", 4)])
def test_zeggs_dims_vs_oracle(gpu, prec, kset, B):
    """ZEGGS dims in the sets `auto` picks at batch 1 / 16 / 48 (asserted) and TILE in bf16w2: a 40-step DDPM chain and DDIM-50 (eta 0.5) with
    root + lower body held for all frames and, for odd batch elements, everything in frames 0..15.  Rows 0 and 1 (an even and an odd element)
    against the oracle on the unmasked elements; the masked elements of EVERY row bit-exact."""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg = C.ZEGGS
    y48 = synth_window_inputs(cfg, 48, window=1, clip0=2, seed_pose_scale=0.3)
    mask48, motion48 = _edit_mask(cfg, 48), _motion(cfg, 48)
    y = {k: (v[:B] if k != "mask_local" else v) for k, v in y48.items()}
    mask, motion = mask48[:B], motion48[:B]
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    m = _model(cfg, prec, max_batch=B)
    if prec == "bf16w2":
        m.set_kernel_set(kset)
    d, d50 = create_gaussian_diffusion(), create_gaussian_diffusion("ddim50")
    d.manual_seed(31, 7).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=998)
    without_keys = (m.last_sample_path(), m.last_sample_fence_free())      # how this configuration is submitted without the keys
    assert without_keys[0] == "aql"
    for name in ("ddpm", "ddim"):
        if name == "ddpm":
            s = np.asarray(d.manual_seed(31, 7).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), skip_timesteps=960))
        else:
            s = np.asarray(d50.manual_seed(31, 8).ddim_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), eta=0.5))
        assert m.last_kernel_set() == kset and (m.last_sample_path(), m.last_sample_fence_free()) == without_keys
        assert np.isfinite(s).all() and np.array_equal(s[mask], motion[mask])
        for b in sorted({0, min(1, B - 1)}):
            r = _zeggs_oracle(name, b, y48, mask48, motion48)
            free = ~mask[b]
            e = rel_l2(s[b][free], r[0][free])
            print(f"inpaint zeggs {prec} {kset} B={B} {name} row {b}: rel-L2 of the unmasked elements = {e:.3e}")
            assert e < _bound(prec, kset, name, b), (name, b, e)


def test_beat_dims_fused_guidance_vs_oracle(gpu):
    """BEAT dims, batch 8 with fused guidance (max_batch 16, the set `auto` picks): the constraint acts on the COMBINED output and is indexed
    by the conditional element; 12 DDPM steps against the oracle's guided loop with the same wrapper"""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    cfg, B = C.BEAT, 8
    m = _model(cfg, "bf16", max_batch=2 * B)
    ref = MDMOracle(synth_state_dict(cfg, 20240), cfg)
    y = synth_window_inputs(cfg, B, window=1, clip0=2, seed_pose_scale=0.3)
    scale = np.linspace(0.5, 2.5, B).astype(np.float32)
    mask, motion = _edit_mask(cfg, B), _motion(cfg, B)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    d = create_gaussian_diffusion().manual_seed(3, 9)
    yy = dict(_y(y, mask, motion)["y"], scale=scale)
    s = np.asarray(d.p_sample_loop(ClassifierFreeSampleModel(m), shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=988))
    assert m.last_sample_path() == "aql" and m.last_sample_fence_free() and np.isfinite(s).all()
    assert np.array_equal(s[mask], motion[mask])
    for k, b in enumerate((0, B - 1)):
        yb = dict(_rows(y, b), scale=scale[b:b + 1])
        r = sampler.p_sample_loop(OracleDiffusion(), sampler.CFGModel(ref), (1,) + shape[1:], lambda k, b=b: philox.normal_bj1t(shape, 3, k, 9)[b:b + 1],
                                  {"y": yb}, skip_timesteps=988, denoised_fn=inpaint_fn(mask[b:b + 1], motion[b:b + 1]))
        free = ~mask[b]
        e = rel_l2(s[b][free], r[0][free])
        print(f"inpaint beat guided B={B} row {b}: rel-L2 of the unmasked elements = {e:.3e}")
        assert e < _bound("bf16", "beat-guided", "ddpm", k), (b, e)


def test_lanes_each_with_its_own_constraint(gpu):
    """4 lanes x batch 4, every lane its own mask and motion: each lane bit-identical to the same lane sampled alone (the lane contract).  Then the
    same call with the keys left out for lane 3 alone: that lane is back to its unconstrained chain, the other three keep theirs."""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    cfg, NL, B = C.ZEGGS, 4, 4
    m = _model(cfg, "bf16", max_batch=B)
    lanes = [m] + [m.clone() for _ in range(NL - 1)]
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    d = create_gaussian_diffusion()
    mks = []
    for ln in range(NL):
        y = synth_window_inputs(cfg, B, window=1, clips=list(range(B * ln, B * ln + B)), seed_pose_scale=0.2)
        mask = np.roll(_edit_mask(cfg, B), 7 * ln, axis=3)
        mask[:, ln::NL] = True
        mks.append(_y(y, mask, _motion(cfg, B, seed=50 + 10 * ln)))
    assert len({mk["y"]["inpainting_mask"].tobytes() for mk in mks}) == NL
    off3 = mks[:3] + [{"y": {k: v for k, v in mks[3]["y"].items() if k not in ("inpainting_mask", "inpainted_motion")}}]
    for which, n_on in ((mks, 4), (off3, 3)):
        multi = d.manual_seed(11, 0).p_sample_loop_multi(lanes, shape, which, seeds=[11] * NL, stream_ids=list(range(NL)), skip_timesteps=990)
        assert all(ln.last_sample_path() == "aql" and ln.last_sample_fence_free() for ln in lanes)
        assert [ln.inpainting for ln in lanes] == [True] * n_on + [False] * (NL - n_on)
        for ln in range(NL):
            alone = np.asarray(d.manual_seed(11, ln).p_sample_loop(lanes[ln], shape, clip_denoised=False, model_kwargs=which[ln], skip_timesteps=990))
            assert np.array_equal(np.asarray(multi[ln]), alone), ln
            if ln < n_on:
                mk = which[ln]["y"]
                assert np.array_equal(alone[mk["inpainting_mask"]], mk["inpainted_motion"][mk["inpainting_mask"]])
