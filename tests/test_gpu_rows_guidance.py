"""GPU: classifier-free guidance fused into the ROWS set at the DSG+ widths (latent_dim 384 / 512, bf16).

The last layer keeps the set's own form (k_clip_attn_w + k_ffn<OP>) and the guided streaming pose head k_ws_cfg reads the conditional rows and
their unconditional twins from the fragment-major LayerNorm2 rows: a workgroup takes 32 conditional rows and their 32 twins, which lie
cfg_off = B x 151 rows further down -- never a multiple of 16, so a twin sits in another row tile at another in-tile row.  Batches (the smallest
that reach each hazard): B = 1 (+ 1 twin: the conditional / twin boundary, row 151, lies inside row tile 9 and inside the last 32-row block),
B = 3 (+ 3: the scale changes inside tiles, ragged last conditional block), B = 9 (+ 9: 43 row blocks per weight panel).

Without the feature every guided call below raises NotImplementedError ("kernel set ROWS at the DSG+ widths: no fused guidance").

Bounds: the project's TOL_FWD / TOL_CHAIN for bf16 (1.2e-2 / 2e-2) and the per-row margin of tests/rowcheck.py (2 x the reference error of the
oracle with the device's roundings), as for the guided STREAM case of tests/test_gpu_rows_every_clip.py."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests import rowcheck
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TOL_FWD = {"bf16": 1.2e-2}
TOL_CHAIN = {"bf16": 2e-2}
CFGS = [C.BEATPP, C.TWH]           # variant 5 (y['seed_last']) at K / 16 = 24; latent 512: K / 16 = 32
BATCHES = (1, 3, 9)
_SD, _ORACLE_OUT, _DEV = {}, {}, {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


def _sd(cfg):
    if cfg.name not in _SD:
        _SD[cfg.name] = synth_state_dict(cfg, 20240)
    return _SD[cfg.name]


def _model(cfg, max_batch, kset="rows", prec="bf16"):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision=prec, max_batch=max_batch, device=0).set_kernel_set(kset)
    m.load_state_dict(_sd(cfg))
    return m


def _scale(B):
    """distinct per clip, 0.0 / 1.0 / 2.5 among them (B = 1: 2.5)"""
    return np.asarray([2.5, 0.0, 1.0, 0.5, 1.75, 3.0, 0.25, 1.5, 2.0][:B], np.float32)


def _oracle_out(cfg, B, kind, uncond):
    """One oracle's output for rowcheck.case_inputs(cfg, B): computed once, shared, read-only."""
    key = (cfg.name, B, kind, uncond)
    if key not in _ORACLE_OUT:
        x, ts, y = rowcheck.case_inputs(cfg, B)
        o = rowcheck.oracle(cfg, _sd(cfg), kind)(x, [int(t) for t in ts], y, uncond_info=uncond)
        o.setflags(write=False)
        _ORACLE_OUT[key] = o
    return _ORACLE_OUT[key]


def _guided(cfg, B, kind):
    s = _scale(B).reshape(-1, 1, 1, 1)
    return _oracle_out(cfg, B, kind, True) + s * (_oracle_out(cfg, B, kind, False) - _oracle_out(cfg, B, kind, True))


def _device_out(cfg, B):
    """The guided ROWS forward of rowcheck.case_inputs(cfg, B) through the wrapper: one per (dims, B), shared, read-only."""
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    key = (cfg.name, B)
    if key not in _DEV:
        x, ts, y = rowcheck.case_inputs(cfg, B)
        m = _model(cfg, 2 * B)
        out = np.asarray(ClassifierFreeSampleModel(m)(x, ts, dict(y, scale=_scale(B))))
        assert m.last_kernel_set() == "rows" and out.shape == x.shape
        out.setflags(write=False)
        _DEV[key] = out
    return _DEV[key]


def _rows(y, sl, B):
    return {k: (v[sl] if v is not None and v.shape[0] == B else v) for k, v in y.items()}


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: c.name)
@pytest.mark.parametrize("B", BATCHES)
def test_guided_forward_every_clip_and_every_row(gpu, cfg, B):
    """One guided forward per B: every clip against uncond + s (cond - uncond) of two MDMOracle evaluations at TOL_FWD, every (clip, frame) row
    within rowcheck's bf16 margin of the same combination of the rounded oracle's two evaluations."""
    out = _device_out(cfg, B)
    want = _guided(cfg, B, "fp32")
    for b in range(B):
        e = rel_l2(out[b:b + 1], want[b:b + 1])
        print(f"ROWS guidance {cfg.name} B={B} clip {b} scale {_scale(B)[b]}: rel-L2 {e:.3e}")
        assert e < TOL_FWD["bf16"], (cfg.name, B, b, e)
    worst = rowcheck.assert_rows_within(out, want, _guided(cfg, B, "bf16"), rowcheck.MARGIN["bf16"], f"{cfg.name} bf16 rows guidance {B} + {B}")
    print(f"ROWCHECK {cfg.name} bf16 rows guidance batch {B} + {B} twins: {B * cfg.n_poses} rows, worst at {worst:.2f} x its reference error")


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: c.name)
def test_guided_rows_are_batch_independent_and_scale_0_1_are_the_plain_forwards(gpu, cfg):
    """Clips 1..2 of the B = 9 call are the bits a max_batch = 4 handle gives those two clips (+ twins) in ROWS.  Scale 0.0 leaves the unconditional
    twin's plain ROWS forward, scale 1.0 the conditional one: `u + 0 (c - u)` is u exactly, `u + (c - u)` rounds twice in fp32 (a few 1e-7 relative,
    asserted at 1e-5, far inside "bf16 noise") -- and against the un-guided kernel (k_ws<OUT>: the same k sums) nothing else differs."""
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    B = 9
    x, ts, y = rowcheck.case_inputs(cfg, B)
    out, sc = _device_out(cfg, B), _scale(B)
    small = _model(cfg, 4)
    two = np.asarray(ClassifierFreeSampleModel(small)(x[1:3], ts[1:3], dict(_rows(y, slice(1, 3), B), scale=sc[1:3])))
    assert small.last_kernel_set() == "rows" and np.array_equal(two, out[1:3])
    assert sc[1] == 0.0 and sc[2] == 1.0
    plain = _model(cfg, 2)
    u = np.asarray(plain(x[1:2], ts[1:2], _rows(y, slice(1, 2), B), uncond_info=True))
    c = np.asarray(plain(x[2:3], ts[2:3], _rows(y, slice(2, 3), B)))
    assert plain.last_kernel_set() == "rows"
    e0, e1 = rel_l2(out[1:2], u), rel_l2(out[2:3], c)
    print(f"ROWS guidance {cfg.name}: scale 0 vs the plain unconditional forward {e0:.3e}, scale 1 vs the plain conditional forward {e1:.3e}")
    assert e0 < 1e-5 and e1 < TOL_FWD["bf16"]


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: c.name)
def test_guided_chains_vs_oracle(gpu, cfg):
    """B = 3 (+ 3 twins): a 12-step DDPM chain and DDIM-50 from skip_timesteps = 40 (10 steps) on fence-free AQL packets in ROWS against the oracle's
    loops driven with the oracle's guidance wrapper -- clip 0 (scale 2.5: the unconditional twin enters with weight -1.5, so a wrong twin row, a twin
    state that drifts over the steps or a wrong scale index shows) and clip 2 (scale 1.0, the last clip: the ragged last block).  The oracle runs the
    two clips as one batch of its own (its clips are independent)."""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    from oracle import philox, sampler
    from oracle.schedule import OracleDiffusion
    B, bs = 3, [0, 2]
    ref = sampler.CFGModel(rowcheck.oracle(cfg, _sd(cfg), "fp32"))
    y = synth_window_inputs(cfg, B, window=1, clip0=2, seed_pose_scale=0.2)
    sc = _scale(B)
    assert sc[0] == 2.5 and sc[2] == 1.0
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    m = _model(cfg, 2 * B)
    w = ClassifierFreeSampleModel(m)
    yb = dict(_rows(y, bs, B), scale=sc[bs])
    got = np.asarray(create_gaussian_diffusion().manual_seed(21, 3).p_sample_loop(w, shape, clip_denoised=False, model_kwargs={"y": dict(y, scale=sc)}, skip_timesteps=988))
    assert m.last_kernel_set() == "rows" and m.last_sample_path() == "aql"
    want = sampler.p_sample_loop(OracleDiffusion(), ref, (len(bs),) + shape[1:], lambda k: philox.normal_bj1t(shape, 21, k, 3)[bs], {"y": yb}, skip_timesteps=988)
    errs = [rel_l2(got[b:b + 1], want[i:i + 1]) for i, b in enumerate(bs)]
    print(f"ROWS guidance {cfg.name} DDPM 12 steps, clips {bs} (scales {sc[bs]}): rel-L2 {errs[0]:.3e} {errs[1]:.3e}")
    assert max(errs) < TOL_CHAIN["bf16"], errs
    d50 = create_gaussian_diffusion("ddim50")
    got = np.asarray(d50.manual_seed(22, 4).ddim_sample_loop(w, shape, clip_denoised=False, model_kwargs={"y": dict(y, scale=sc)}, skip_timesteps=40))
    assert m.last_kernel_set() == "rows" and m.last_sample_path() == "aql"
    want = sampler.ddim_sample_loop(OracleDiffusion(timestep_respacing="ddim50"), ref, (len(bs),) + shape[1:], lambda k: philox.normal_bj1t(shape, 22, k, 4)[bs],
                                    {"y": yb}, skip_timesteps=40)
    errs = [rel_l2(got[b:b + 1], want[i:i + 1]) for i, b in enumerate(bs)]
    print(f"ROWS guidance {cfg.name} DDIM-50 from skip 40, clips {bs} (scales {sc[bs]}): rel-L2 {errs[0]:.3e} {errs[1]:.3e}")
    assert max(errs) < TOL_CHAIN["bf16"], errs


def test_guided_chain_with_inpainting_on_half_the_joints(gpu):
    """B = 3 at the BEAT++ dims, y['inpainting_mask'] on the first half of the pose features: the constraint acts on the COMBINED prediction and is
    indexed by the conditional element.  The last DDPM step has posterior_mean_coef1 == 1 and adds no noise, so masked elements ARE the motion; the
    unmasked ones stay under the bound of the unconstrained chain."""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    from oracle import philox, sampler
    from oracle.schedule import OracleDiffusion
    from tests.test_inpaint_golden import inpaint_fn
    cfg, B, b = C.BEATPP, 3, 1
    ref = sampler.CFGModel(rowcheck.oracle(cfg, _sd(cfg), "fp32"))
    y = synth_window_inputs(cfg, B, window=1, clip0=2, seed_pose_scale=0.2)
    sc = np.asarray([2.5, 1.5, 0.5], np.float32)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    mask = np.zeros(shape, bool)
    mask[:, :cfg.njoints // 2] = True
    motion = np.stack([(0.8 * np.random.RandomState(1818 + k).randn(*shape[1:])).astype(np.float32) for k in range(B)])
    m = _model(cfg, 2 * B)
    yy = dict(y, scale=sc, inpainting_mask=mask, inpainted_motion=motion)
    got = np.asarray(create_gaussian_diffusion().manual_seed(5, 6).p_sample_loop(ClassifierFreeSampleModel(m), shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=988))
    assert m.last_kernel_set() == "rows" and m.last_sample_path() == "aql"
    assert np.array_equal(got[mask], motion[mask])
    yb = dict(_rows(y, slice(b, b + 1), B), scale=sc[b:b + 1])
    want = sampler.p_sample_loop(OracleDiffusion(), ref, (1,) + shape[1:], lambda k: philox.normal_bj1t(shape, 5, k, 6)[b:b + 1], {"y": yb}, skip_timesteps=988,
                                 denoised_fn=inpaint_fn(mask[b:b + 1], motion[b:b + 1]))
    free = ~mask[b]
    e = rel_l2(got[b][free], want[0][free])
    print(f"ROWS guidance beatpp inpainting, clip {b}: rel-L2 of the unmasked elements {e:.3e}")
    assert e < TOL_CHAIN["bf16"], e


def test_guided_lanes_reproduce_themselves_alone(gpu):
    """Two lanes x (3 + 3 twins) through p_sample_loop_multi: each lane bit-identical to the lane sampled alone."""
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    cfg, B, NL = C.BEATPP, 3, 2
    m = _model(cfg, 2 * B)
    lanes = [m, m.clone()]
    wrapped = [ClassifierFreeSampleModel(ln) for ln in lanes]
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    ys = [{"y": dict(synth_window_inputs(cfg, B, window=w, clip0=B * w, seed_pose_scale=0.2), scale=_scale(B) + 0.125 * w)} for w in range(NL)]
    d = create_gaussian_diffusion()
    multi = d.manual_seed(9, 0).p_sample_loop_multi(wrapped, shape, ys, seeds=[9] * NL, stream_ids=list(range(NL)), skip_timesteps=992)
    assert all(ln.last_kernel_set() == "rows" and ln.last_sample_path() == "aql" for ln in lanes)
    for i in range(NL):
        alone = d.manual_seed(9, i).p_sample_loop(wrapped[i], shape, clip_denoised=False, model_kwargs=ys[i], skip_timesteps=992)
        assert lanes[i].last_kernel_set() == "rows" and np.array_equal(np.asarray(multi[i]), np.asarray(alone)), i


def test_bf16w2_rows_under_guidance_is_still_refused(gpu):
    """Out of scope here and unchanged: a bf16w2 handle pinned to ROWS refuses a guided call (its guided last layer has no two-register form)."""
    from diffusestylegesture_amd.model import ClassifierFreeSampleModel
    cfg, B = C.ZEGGS, 2
    m = _model(cfg, 2 * B, prec="bf16w2")
    x, ts, y = rowcheck.case_inputs(cfg, B)
    with pytest.raises(NotImplementedError):
        ClassifierFreeSampleModel(m)(x, ts, dict(y, scale=_scale(B)))
