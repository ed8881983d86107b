"""CPU: motion inpainting (y['inpainting_mask'] / y['inpainted_motion'], gaussian_diffusion.py:317-321) through the product sources under the
SIMT emulator -- the transpose kernel, the select in the pose-head epilogue, the host sequencing and the Python key handling -- against the
reference's own loops (G18).  The real-hardware tests are tests/test_gpu_inpaint.py (-m gpu); the generic loop (a plain callable as the model,
or a denoised_fn) is checked there too: its update kernels take device tensors, which torch does not have under the emulator -- as for the
hook tests of G17 (test_emu_parity.py: "denoised_fn / cond_fn run step by step on the device").  Of the generic loop only the shape check, which
comes before its first library call, runs here."""
import os
import re

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
from diffusestylegesture_amd.model import DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.test_emu_parity import TOL
from tests.util import rel_l2

TOL_CHAIN_FP32 = 3 * TOL["fp32"]      # the emulator's fp32 chain bound (test_emu_parity.test_chains_tiny)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_inpaint_tiny.npz"))


@pytest.fixture(scope="module")
def tiny(emu_lib, g18):
    sd = synth_state_dict(C.TINY, int(g18["wseed"]))

    def make(prec="fp32", B=2):
        m = DSGDenoiser(C.TINY, precision=prec, max_batch=B, library=emu_lib)
        m.load_state_dict(sd)
        return m
    y = synth_window_inputs(C.TINY, 2, window=2, seed_pose_scale=0.3)
    return make, y, (2, C.TINY.njoints, 1, C.TINY.n_poses)


def _y(y, mask, motion):
    return {"y": dict(y, inpainting_mask=mask, inpainted_motion=motion)}


def test_fused_chains_vs_reference(tiny, emu_lib, g18):
    """the fused DDPM (with and without the clamp) and DDIM chains with the keys set reproduce the reference's loops; where the mask is
    set and the clamp is off the final sample IS the motion: at loop index 0 posterior_mean_coef1 == 1, coef2 == 0 and no noise is added
    (DDPM), alphas_cumprod_prev[0] == 1 gives k3 = 1, k4 = k5 = 0 (DDIM)"""
    make, y, shape = tiny
    m, motion = make(), g18["motion"]
    seed = int(g18["noise_seed"])
    d, d50 = create_gaussian_diffusion(library=emu_lib), create_gaussian_diffusion("ddim50", library=emu_lib)
    mask = g18["mask_joints"]
    s = d.manual_seed(seed, 21).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), skip_timesteps=800)
    e = rel_l2(s, g18["ddpm_joints_skip800"])
    print("ddpm joints", e)
    assert e < TOL_CHAIN_FP32 and np.array_equal(s[mask], motion[mask])
    mask = g18["mask_frames"]
    s = d.manual_seed(seed, 22).p_sample_loop(m, shape, clip_denoised=True, model_kwargs=_y(y, mask, motion), skip_timesteps=800)
    e = rel_l2(s, g18["ddpm_frames_clip_skip800"])
    print("ddpm frames clip", e)
    assert e < TOL_CHAIN_FP32 and np.array_equal(s[mask], np.clip(motion, -1, 1)[mask])      # inpainting first, then the clamp
    mask = g18["mask_checker"]
    s = d50.manual_seed(seed, 23).ddim_sample_loop(m, shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), eta=0.5)
    e = rel_l2(s, g18["ddim50_checker_eta05"])
    print("ddim50 checker", e)
    assert e < TOL_CHAIN_FP32 and np.array_equal(s[mask], motion[mask])


def test_progressive_forms_bit_identical(tiny, emu_lib, g18, monkeypatch):
    """the generator forms run the chain in pieces (`_prepare` per chunk): the same samples as the one-call loops, bit for bit"""
    make, y, shape = tiny
    m, motion, mask = make(), g18["motion"], g18["mask_checker"]
    d, d50 = create_gaussian_diffusion(library=emu_lib), create_gaussian_diffusion("ddim50", library=emu_lib)
    monkeypatch.setattr(type(d), "PROGRESSIVE_CHUNK", 5)
    mk = _y(y, mask, motion)
    one = d.manual_seed(5, 1).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=mk, skip_timesteps=988)
    outs = [o["sample"] for o in d.manual_seed(5, 1).p_sample_loop_progressive(m, shape, clip_denoised=False, model_kwargs=mk, skip_timesteps=988)]
    assert len(outs) == 12 and np.array_equal(outs[-1], one)
    one = d50.manual_seed(5, 2).ddim_sample_loop(m, shape, clip_denoised=False, model_kwargs=mk, eta=0.5, skip_timesteps=38)
    outs = [o["sample"] for o in d50.manual_seed(5, 2).ddim_sample_loop_progressive(m, shape, clip_denoised=False, model_kwargs=mk, eta=0.5,
                                                                                    skip_timesteps=38)]
    assert len(outs) == 12 and np.array_equal(outs[-1], one)


def test_const_noise_shares_the_noise_not_the_constraint(tiny, emu_lib, g18):
    """const_noise gives every batch element the step noise of element 0; each element keeps its own mask and motion.  Yardstick: the oracle's
    const_noise loop with the constraint as its denoised_fn (tests/test_inpaint_golden.py), at the emulator's fp32 chain bound."""
    from oracle import sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    from tests.test_inpaint_golden import inpaint_fn
    make, y, shape = tiny
    motion, mask = g18["motion"], g18["mask_frames"]            # frames 0..5 of element 0, frames 9..16 of element 1
    assert not np.array_equal(mask[0], mask[1]) and not np.array_equal(motion[0], motion[1])
    d = create_gaussian_diffusion(library=emu_lib)
    s = d.manual_seed(77, 5).p_sample_loop(make(), shape, clip_denoised=False, model_kwargs=_y(y, mask, motion), skip_timesteps=994, const_noise=True)
    ref = MDMOracle(synth_state_dict(C.TINY, int(g18["wseed"])), C.TINY)
    want = {cn: sampler.p_sample_loop(OracleDiffusion(), ref, shape, sampler.philox_noise_fn(shape, 77, 5), {"y": y}, skip_timesteps=994,
                                      const_noise=cn, denoised_fn=inpaint_fn(mask, motion)) for cn in (True, False)}
    e = rel_l2(s, want[True])
    print("const_noise + constraint", e)
    assert e < TOL_CHAIN_FP32 and rel_l2(s, want[False]) > 1e-3      # (six late steps: sharing the noise moves element 1 by 2.8e-3)
    assert np.array_equal(s[mask], motion[mask])


def test_key_handling(tiny, emu_lib, g18):
    make, y, shape = tiny
    motion, mask = g18["motion"], g18["mask_frames"]
    d = create_gaussian_diffusion(library=emu_lib)
    run = lambda m, mk: d.manual_seed(9, 4).p_sample_loop(m, shape, clip_denoised=False, model_kwargs=mk, skip_timesteps=994)
    fresh = run(make(), {"y": y})
    m = make()
    on = run(m, _y(y, mask, motion))
    assert m.inpainting and not np.array_equal(on, fresh) and np.array_equal(on[mask], motion[mask])
    # a call without the keys after a call with them: the constraint is gone (sticky in the handle, switched off by _prepare)
    assert np.array_equal(run(m, {"y": y}), fresh) and not m.inpainting
    # one key alone is ignored, as in the reference
    assert np.array_equal(run(m, {"y": dict(y, inpainting_mask=mask)}), fresh)
    assert np.array_equal(run(m, {"y": dict(y, inpainted_motion=motion)}), fresh)
    # uint8 masks, per-element constraints (the two batch elements swapped give the swapped result where rows do not interact: masked part)
    on8 = run(m, _y(y, mask.astype(np.uint8) * 255, motion))
    assert np.array_equal(on8, on)
    # a wrong shape raises ValueError (the reference asserts), for either key, in the fused and the generic loop
    for bad in (_y(y, mask[:, :-1], motion), _y(y, mask, motion[..., :-1]), _y(y, mask[:1], motion[:1])):
        with pytest.raises(ValueError, match=r"y\['inpaint\w+'\] shape"):
            run(m, bad)
    # the C ABI: exactly one NULL pointer, B > max_batch -> DSG_E_INVALID; both NULL switches off; a clone starts without a constraint
    from diffusestylegesture_amd import lib as L
    mb, vb = L.Buf(mask, "uint8"), L.Buf(motion)
    f = emu_lib.cdll.dsg_set_inpainting
    assert f(m.handle, mb.p, None, 2, None) == -1                  # DSG_E_INVALID
    assert f(m.handle, None, vb.p, 2, None) == -1
    assert f(m.handle, mb.p, vb.p, 3, None) == -1
    assert f(m.handle, mb.p, vb.p, 2, None) == 0
    c = m.clone()
    assert np.array_equal(run(c, {"y": y}), fresh)                 # (the clone holds no constraint although its source does)
    m.set_cond(y, 2)                                              # dsg_set_window_cond leaves the constraint alone
    m.inpainting = True                                           # (set through the bare ABI above)
    assert np.array_equal(run(m, _y(y, mask, motion)), on)
    assert f(m.handle, None, None, 0, None) == 0
    # a constraint of another batch than the sampling call is an error, not an out-of-range read
    m1 = make(B=2)
    assert f(m1.handle, mb.p, vb.p, 1, None) == 0
    m1.inpainting = False
    with pytest.raises(ValueError):
        run(m1, {"y": y})
    # the generic loop (here: a denoised_fn) checks the shapes of both keys before its first library call (which, under the emulator, would
    # refuse torch's host tensors with another ValueError: hence the match)
    import torch
    for bad in (_y(y, mask[:, :-1], motion), _y(y, mask, motion[..., :-1])):
        yt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in bad["y"].items()}
        with pytest.raises(ValueError, match=r"y\['inpaint\w+'\] shape"):
            d.manual_seed(9, 4).p_sample_loop(m, shape, clip_denoised=False, denoised_fn=lambda x: x, model_kwargs={"y": yt}, skip_timesteps=994)


def _resource_report():
    """the register report of the code object, read as test_abi.test_no_kernel_spills_to_scratch reads it: the file `make` writes next to the
    code object (csrc/dsg_kernels.resources.txt), or, when that is missing or older than a kernel source, the same compile's remarks"""
    import glob
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "diffusestylegesture_amd", "csrc")
    rep = os.path.join(csrc, "dsg_kernels.resources.txt")
    srcs = [os.path.join(csrc, "dsg_hip.cpp")] + sorted(glob.glob(os.path.join(csrc, "*.h")))      # (every header: dsg_stream.h holds k_ws)
    if os.path.exists(rep) and os.path.getmtime(rep) >= max(os.path.getmtime(f) for f in srcs):
        return open(rep).read()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no register report and no hipcc to write one"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "--cuda-device-only",
                          "-c", srcs[0], "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


def test_every_instantiation_without_scratch_and_one_new_kernel(hip_lib_path):
    """the rebuilt code object: ScratchSize == 0 for every kernel (the AQL packets carry private_segment_size 0), and the transpose kernel is there"""
    text = _resource_report()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) and len(names) > 40
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert sum("k_inp_in" in n for n in names) == 1
    # the STREAM pose head k_ws<EPI_OUT, K / 16, true> at K = 128 / 256 keeps the four waves per SIMD it had before the select (DESIGN s1: 122 -> 125
    # and 126 -> 128 registers under its bound of four workgroups per CU)
    occ = dict(zip(names, (int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", text))))
    head = [n for n in names if re.search(r"k_wsILi4ELi(8|16)ELb1E", n)]
    assert len(head) == 2 and all(occ[n] >= 4 for n in head), [(n, occ[n]) for n in head]
