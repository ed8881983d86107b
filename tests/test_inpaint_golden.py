"""CPU: the unchanged oracle reproduces the reference's inpainting loops (G18, tests/golden/make_goldens_inpaint.py) when it is driven with
`denoised_fn = lambda x0: where(mask, motion, x0)` -- the oracle applies denoised_fn to the model's prediction before the clamp, which is where
p_mean_variance applies the constraint (gaussian_diffusion.py:317-321, before :364-370).  This is what licenses the oracle, driven that way, as the
yardstick of the GPU tests at the full dims (tests/test_gpu_inpaint.py).  Bound: the oracle's chain bound of G17."""
import os

import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from oracle import sampler
from oracle.mdm import MDMOracle
from oracle.schedule import OracleDiffusion
from tests.test_oracle_vs_golden import TOL_CHAIN, hook_denoised
from tests.util import rel_l2


def inpaint_fn(mask, motion, then=None):
    """the constraint as a denoised_fn of the oracle; `then`: the caller's own denoised_fn, which the reference applies after it"""
    def fn(x0):
        x0 = np.where(mask, motion, x0).astype(np.float32)
        return x0 if then is None else then(x0)
    return fn


def test_oracle_with_where_as_denoised_fn_reproduces_reference_inpainting(golden_dir):
    g = np.load(os.path.join(golden_dir, "g18_inpaint_tiny.npz"))
    cfg = C.TINY
    m = MDMOracle(synth_state_dict(cfg, int(g["wseed"])), cfg)
    y = synth_window_inputs(cfg, 2, window=2, seed_pose_scale=0.3)
    shape = (2, cfg.njoints, 1, cfg.n_poses)
    mk, motion = {"y": y}, g["motion"]
    d, d50 = OracleDiffusion(), OracleDiffusion(timestep_respacing="ddim50")
    nf = lambda s: sampler.philox_noise_fn(shape, int(g["noise_seed"]), s)
    got = sampler.p_sample_loop(d, m, shape, nf(21), mk, skip_timesteps=800, denoised_fn=inpaint_fn(g["mask_joints"], motion))
    assert rel_l2(got, g["ddpm_joints_skip800"]) < TOL_CHAIN
    assert np.array_equal(got[g["mask_joints"]], motion[g["mask_joints"]])
    got = sampler.p_sample_loop(d, m, shape, nf(22), mk, skip_timesteps=800, clip_denoised=True, denoised_fn=inpaint_fn(g["mask_frames"], motion))
    assert rel_l2(got, g["ddpm_frames_clip_skip800"]) < TOL_CHAIN
    got = sampler.ddim_sample_loop(d50, m, shape, nf(23), mk, eta=0.5, denoised_fn=inpaint_fn(g["mask_checker"], motion))
    assert rel_l2(got, g["ddim50_checker_eta05"]) < TOL_CHAIN
    got = sampler.p_sample_loop(d, m, shape, nf(24), mk, skip_timesteps=800, denoised_fn=inpaint_fn(g["mask_joints"], motion, hook_denoised))
    assert rel_l2(got, g["ddpm_joints_hook_skip800"]) < TOL_CHAIN
    # the fixture is not the unconstrained chain, and the order of the two hooks matters
    assert rel_l2(sampler.p_sample_loop(d, m, shape, nf(21), mk, skip_timesteps=800), g["ddpm_joints_skip800"]) > 1e-2
    swapped = lambda x0: inpaint_fn(g["mask_joints"], motion)(hook_denoised(x0))
    assert rel_l2(sampler.p_sample_loop(d, m, shape, nf(24), mk, skip_timesteps=800, denoised_fn=swapped), g["ddpm_joints_hook_skip800"]) > 1e-2
