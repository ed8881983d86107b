#!/usr/bin/env python3
"""G18: motion inpainting in the reference's own sampling loops (dev container only).

    python tests/golden/make_goldens_inpaint.py      # -> tests/golden/g18_inpaint_tiny.npz

`p_mean_variance` (main/diffusion/gaussian_diffusion.py:317-321) replaces the model's x0 prediction by y['inpainted_motion'] wherever
y['inpainting_mask'] is set -- before denoised_fn, the clamp and the posterior.  This script imports the reference exactly as
`make_goldens.py hooks` (G17) does -- same helpers, tiny dims, batch 2, synthetic weights, the framework's Philox noise injected -- and
runs its loops with the two keys in `y`:

    ddpm_joints_skip800        DDPM, 200 steps, joints 5..19 of every frame held
    ddpm_frames_clip_skip800   the same with clip_denoised=True and a frame range that differs between the two batch elements
    ddim50_checker_eta05       DDIM-50, eta 0.5, checkerboard mask
    ddpm_joints_hook_skip800   the first case + denoised_fn = hook_denoised of G17: pins that inpainting comes first

The motion is drawn from a seeded generator scaled by 0.8, so some values lie outside [-1, 1] and the clamp of the second case bites.
Only outputs, seeds, masks and motions are stored.  The DSG+ tree (BEAT-TWH-main/diffusion/gaussian_diffusion.py:310-314) is checked while
writing to hold the same condition, asserts and select, line for line; it does (the file differs elsewhere, not here).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_goldens as G
from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_window_inputs

MOTION_SEED = 1818


def inpaint_cases(cfg, B):
    """name -> bool mask [B, J, 1, T]"""
    J, T = cfg.njoints, cfg.n_poses
    joints = np.zeros((B, J, 1, T), bool)
    joints[:, 5:20] = True
    frames = np.zeros((B, J, 1, T), bool)
    frames[0, :, :, 0:6] = True
    frames[1, :, :, 9:17] = True
    jj, tt = np.meshgrid(np.arange(J), np.arange(T), indexing="ij")
    checker = np.broadcast_to((((jj + tt) & 1) == 0)[None, :, None, :], (B, J, 1, T)).copy()
    return {"joints": joints, "frames": frames, "checker": checker}


def _same_lines_in_dsgplus():
    def block(path):
        src = open(path).read().splitlines()
        i = next(n for n, line in enumerate(src) if "inpainting_mask" in line)      # (the first mention of the key opens the block)
        return [line.strip() for line in src[i:i + 5]]
    a = block(G.REF + "/main/diffusion/gaussian_diffusion.py")
    b = block(G.REF + "/BEAT-TWH-main/diffusion/gaussian_diffusion.py")
    assert a == b and "inpainted_motion" in a[4], (a, b)


def gen_inpaint():
    _same_lines_in_dsgplus()
    sys.path[:0] = [G.REF + "/main", G.REF + "/main/model"]
    np.float = float
    from utils.model_util import create_gaussian_diffusion
    from diffusion import gaussian_diffusion as gd
    from diffusion.respace import SpacedDiffusion, space_timesteps
    diff = create_gaussian_diffusion()
    d50 = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim50"), betas=gd.get_named_beta_schedule('cosine', 1000, 1.),
                          model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                          loss_type=gd.LossType.MSE, rescale_timesteps=False)
    cfg = C.TINY
    model, _ = G._build_ref_zeggs(cfg)
    B = 2
    y = synth_window_inputs(cfg, B, window=2, seed_pose_scale=0.3)
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    masks = inpaint_cases(cfg, B)
    motion = (0.8 * np.random.RandomState(MOTION_SEED).randn(*shape)).astype(np.float32)
    assert (np.abs(motion) > 1).mean() > 0.1

    def mk(mask):
        yt = G._y_torch(y)
        yt["inpainting_mask"], yt["inpainted_motion"] = torch.from_numpy(mask), torch.from_numpy(motion)
        return {"y": yt}
    g = {"wseed": G.WSEED, "noise_seed": 77, "motion_seed": MOTION_SEED, "motion": motion}
    for k, v in masks.items():
        g["mask_" + k] = v
    with G.NoiseInjector(77, stream=21):
        g["ddpm_joints_skip800"] = diff.p_sample_loop(model, shape, clip_denoised=False, model_kwargs=mk(masks["joints"]),
                                                      skip_timesteps=800, progress=False).numpy()
    with G.NoiseInjector(77, stream=22):
        g["ddpm_frames_clip_skip800"] = diff.p_sample_loop(model, shape, clip_denoised=True, model_kwargs=mk(masks["frames"]),
                                                           skip_timesteps=800, progress=False).numpy()
    with G.NoiseInjector(77, stream=23):
        g["ddim50_checker_eta05"] = d50.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs=mk(masks["checker"]),
                                                         progress=False, eta=0.5).numpy()
    with G.NoiseInjector(77, stream=24):
        g["ddpm_joints_hook_skip800"] = diff.p_sample_loop(model, shape, clip_denoised=False, denoised_fn=G.hook_denoised,
                                                           model_kwargs=mk(masks["joints"]), skip_timesteps=800, progress=False).numpy()
    # what the fixture pins: the constraint is met exactly without the clamp, clamped with it, and scaled by the hook that runs after it
    m = masks["joints"]
    assert np.array_equal(g["ddpm_joints_skip800"][m], motion[m])
    m = masks["frames"]
    assert np.array_equal(g["ddpm_frames_clip_skip800"][m], np.clip(motion, -1, 1)[m])
    m = masks["checker"]
    assert np.array_equal(g["ddim50_checker_eta05"][m], motion[m])
    m = masks["joints"]
    assert np.allclose(g["ddpm_joints_hook_skip800"][m], G.hook_denoised(motion)[m], atol=1e-6)
    np.savez_compressed(os.path.join(HERE, "g18_inpaint_tiny.npz"), **g)
    print("G18 ok", {k: float(np.abs(v).mean()) for k, v in g.items() if k.startswith("dd")})


if __name__ == "__main__":
    gen_inpaint()
