"""GPU: the ROWS kernel set in bf16w2 at the DSG+ widths (latent_dim 384 / 512) -- 16 x 16 tile pose embedding with the embedding rows written as a
hi + lo pair, per layer the QKV GEMM on those pairs (k_gemm_qkv_pair) + k_attn + k_ffn<OP> on one 16-row tile (two-register fragments, W_o leading
the ring, operand fragments re-read from LDS), 16 x 16 tile pose head on the pair rows with K = 384 / 512.

BEAT / TWH have 151 token rows per clip.  Batch 3 is 453 rows: 28 tiles + 5 rows, clip boundaries inside tiles 9 and 18; batch 2 is 302 rows:
18 tiles + 14 rows, the boundary inside tile 9.  A ROWS workgroup owns one 16-row tile or one (query tile, head, clip), so nothing else depends on
the batch.

Measured on MI355X: DESIGN.md s2 (the ROWS bf16w2 rows of the DSG+ tables)."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests import rowcheck
from tests import stepcheck as S
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

PREC, KSET = "bf16w2", "rows"
CAP_CHAIN = 1.5e-3       # the cap the project holds bf16w2 chains to (tests/test_gpu_inpaint.py: CAP_UNCONSTRAINED["bf16w2"])
TOL_FWD = 8e-4           # the whole-output bound of bf16w2 TILE at these dims (tests/test_gpu_round5.py)
_SD, _ORACLE_OUT, _DEV_OUT, _CASE = {}, {}, {}, {}


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


def _model(cfg, max_batch, kset=KSET):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision=PREC, max_batch=max_batch, device=0).set_kernel_set(kset)
    m.load_state_dict(_sd(cfg))
    return m


def _oracle_out(cfg, B, mask_form, kind):
    """One oracle's output for the inputs of (cfg, B, mask_form): computed once, shared by the tests that need it, read-only."""
    key = (cfg.name, B, mask_form, kind)
    if key not in _ORACLE_OUT:
        x, ts, y = rowcheck.case_inputs(cfg, B, mask_form)
        o = rowcheck.oracle(cfg, _sd(cfg), kind)(x, [int(t) for t in ts], y)
        o.setflags(write=False)
        _ORACLE_OUT[key] = o
    return _ORACLE_OUT[key]


def _device_out(cfg, B, mask_form):
    """The device's forward of those inputs on the pinned set (asserted to be the set that ran): once per case, read-only."""
    key = (cfg.name, B, mask_form)
    if key not in _DEV_OUT:
        x, ts, y = rowcheck.case_inputs(cfg, B, mask_form)
        m = _model(cfg, B)
        out = np.asarray(m(x, ts, y))
        assert m.last_kernel_set() == KSET
        out.setflags(write=False)
        _DEV_OUT[key] = out
    return _DEV_OUT[key]


ROW_CASES = [(n, 3, mf) for n in ("beat", "twh") for mf in rowcheck.MASK_FORMS] + [
    ("beatpp", 2, "ones"),       # variant 5 through the same kernels
    ("beatv2", 2, "ones"),       # pose width 1141 at latent 384
    ("twh3", 2, "ones")]         # variant 3 at 512


@pytest.mark.parametrize("name,B,mask_form", ROW_CASES, ids=["-".join(str(f) for f in c) for c in ROW_CASES])
def test_every_row_of_every_clip(gpu, name, B, mask_form):
    """One forward of batch B: all B x T rows within 2 x max(that row's reference error, the batch's median), the reference being the oracle with
    the bf16w2 roundings of ROWS (rowcheck.ref_kind: the embedding output a pair)."""
    cfg = C.CONFIGS[name]
    out = _device_out(cfg, B, mask_form)
    want, ref = _oracle_out(cfg, B, mask_form, "fp32"), _oracle_out(cfg, B, mask_form, rowcheck.ref_kind(PREC, KSET))
    worst = rowcheck.assert_rows_within(out, want, ref, rowcheck.MARGIN[PREC], f"{name} {PREC} {KSET} batch {B} mask {mask_form}")
    print(f"ROWCHECK {name} {PREC} {KSET} batch {B} mask {mask_form}: {B * cfg.n_poses} rows, worst at {worst:.2f} x its reference error")


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_whole_output_against_the_fp32_oracle(gpu, name):
    """rel-L2 of the batch-3 output below 8e-4, the bound bf16w2 TILE is held to at these dims."""
    cfg = C.CONFIGS[name]
    e = rel_l2(_device_out(cfg, 3, "ones"), _oracle_out(cfg, 3, "ones", "fp32"))
    print(f"FORWARD {name} {PREC} {KSET} batch 3: rel-L2 against the fp32 oracle {e:.3e} (bound {TOL_FWD:g})")
    assert e < TOL_FWD


def _case(name, B):
    """The step-check case of (name, B): model, schedules and inputs built once and kept while its tests run (one case at a time)."""
    key = (name, B)
    if key not in _CASE:
        _CASE.clear()
        cfg = C.CONFIGS[name]
        y = synth_window_inputs(cfg, B, window=1, clip0=3, seed_pose_scale=0.2)
        _CASE[key] = S.Case(_model(cfg, B), KSET, B, y, tag=f"{name} {PREC} {KSET} {B}")
    return _CASE[key]


STEP_MODES = [m for m in S.MODES if m[0] in ("ddpm", "ddim-eta1")]


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_one_step_at_every_loop_index(gpu, name):
    """The last DDPM step is the forward bit for bit; one DDPM and one DDIM step at each of stepcheck.loop_indices, every element within 8 u S."""
    c = _case(name, 3)
    c.check_last_step_is_forward()
    w = c.check_all(modes=STEP_MODES)
    print(f"STEPCHECK {c.tag} one step: worst element / bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_two_steps_at_the_loop_indices(gpu, name):
    """Two steps in one call == two one-step calls, and the second step within 8 u S of the float64 step on the device's own forward -- DDPM and
    DDIM, from each of stepcheck.loop_indices that has a step behind it."""
    c = _case(name, 3)
    for mname, mode, sched, args in STEP_MODES:
        n = c.odiff[sched].num_timesteps
        w = {i: c.check_two_steps(mname, mode, sched, args, i=i) for i in S.loop_indices(n) if i + 1 < n}
        print(f"STEPCHECK {c.tag} {mname} second of two steps: worst element / bound " + ", ".join(f"i={i} {v:.3f}" for i, v in w.items()))


def _diffusion():
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    return create_gaussian_diffusion()


def test_short_chain_against_the_fp32_oracle_and_clone(gpu):
    """10 DDPM steps at BEAT batch 3 against the fp32 oracle's chain on the same Philox noise, below the bf16w2 chain cap; a clone() of the handle
    reproduces the chain bit for bit."""
    from oracle import sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    cfg, B = C.BEAT, 3
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    y = synth_window_inputs(cfg, B, window=1, clip0=3, seed_pose_scale=0.2)
    m = _model(cfg, B)
    d = _diffusion()
    got = np.asarray(d.manual_seed(21, 3).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=990))
    assert m.last_kernel_set() == KSET
    want = sampler.p_sample_loop(OracleDiffusion(), MDMOracle(_sd(cfg), cfg), shape, sampler.philox_noise_fn(shape, 21, 3), {"y": y}, skip_timesteps=990)
    e = rel_l2(got, want)
    print(f"CHAIN beat {PREC} {KSET} batch 3, 10 DDPM steps: rel-L2 against the fp32 oracle's chain {e:.3e} (cap {CAP_CHAIN:g})")
    assert np.isfinite(got).all() and e < CAP_CHAIN
    c = m.clone()
    again = np.asarray(d.manual_seed(21, 3).p_sample_loop(c, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=990))
    assert c.last_kernel_set() == KSET and np.array_equal(got, again)


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_lanes_and_clip_streams_bit_identities(gpu, name):
    """Two lanes of batch 2 through p_sample_loop_multi each equal the lane's call alone; with clip_streams, clip 2 of the batch-3 chain equals the
    batch-1 call after manual_seed(seed_2, stream_2).  4 steps each."""
    cfg = C.CONFIGS[name]
    d, skip = _diffusion(), 996
    m2 = _model(cfg, 2)
    lanes = [m2, m2.clone()]
    shape2 = (2, cfg.njoints, 1, cfg.n_poses)
    ys = [{"y": synth_window_inputs(cfg, 2, window=w, clip0=2 * w, seed_pose_scale=0.2)} for w in range(2)]
    multi = d.manual_seed(9, 0).p_sample_loop_multi(lanes, shape2, ys, seeds=[9, 9], stream_ids=[0, 1], skip_timesteps=skip)
    for i in range(2):
        alone = d.manual_seed(9, i).p_sample_loop(lanes[i], shape2, clip_denoised=False, model_kwargs=ys[i], skip_timesteps=skip)
        assert lanes[i].last_kernel_set() == KSET and np.array_equal(np.asarray(multi[i]), np.asarray(alone)), (name, i)
    B = 3
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    y = synth_window_inputs(cfg, B, window=1, clip0=3, seed_pose_scale=0.2)
    seeds, streams = (11, 12, 13), (5, 2 ** 33 + 1, 7)
    m3 = _model(cfg, B)
    got = np.asarray(d.manual_seed(1, 99).p_sample_loop(m3, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip,
                                                        clip_streams=list(zip(seeds, streams))))
    assert m3.last_kernel_set() == KSET
    y1 = {k: (v if k == "mask_local" else v[2:3]) for k, v in y.items()}
    m1 = _model(cfg, 1)
    alone = np.asarray(d.manual_seed(seeds[2], streams[2]).p_sample_loop(m1, (1,) + shape[1:], clip_denoised=False, model_kwargs={"y": y1},
                                                                         skip_timesteps=skip))
    assert m1.last_kernel_set() == KSET and np.array_equal(got[2:3], alone)
