"""CPU: per-clip skip_timesteps in the clip queue (dsg_sample_clip_queue_steps / dsg_clip_queue_plan_steps; the "skip_timesteps" key of
`DSGDiffusion.sample_clip_queue` and `sample.generate_clip_queue[_dsgplus]`) through the product sources under the SIMT emulator.  Fresh
generations and edits of any depth share the slots of one call; every clip must come out bit for bit as dsg_sample_clip produces it alone on a
batch-1 handle with ITS skip_timesteps, under the same named kernel set.  The checks themselves are tests/clip_queue_steps_util.py; the
real-hardware run is tests/test_gpu_clip_queue_steps.py (-m gpu)."""
import pytest

from diffusestylegesture_amd import config as C
from tests import clip_queue_steps_util as U


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mixed_strengths_every_kernel_set(emu_lib, prec):
    """TINY, K = (1, 3, 2, 1, 2) over one lane of B = 2, skips (996, 994, 999, 998, 996) beside the keyword's 996, under every kernel set the
    handle accepts for batch 2 and batch 1: edits A under DDPM with the root shift, edits B under DDIM (eta 0.5) without; the other pairing
    under TILE"""
    sets = U.accepted_sets(emu_lib, C.TINY, prec, 2)
    assert "tile" in sets and len(sets) >= 3, sets
    for ks in sets:
        U.check_mixed(emu_lib, C.TINY, prec, ks)
    U.check_mixed(emu_lib, C.TINY, prec, "tile", cases=U.CROSS)


def test_mixed_strengths_bf16w2_tile(emu_lib):
    U.check_mixed(emu_lib, C.TINY, "bf16w2", "tile")


def test_deep_holds_and_ddim_eta_0(emu_lib):
    U.check_deep_holds(emu_lib)


def test_fresh_beside_edits_four_step_schedule(emu_lib):
    U.check_fresh_beside_edits(emu_lib)


def test_dsgplus_stitching_keep_last_tail(emu_lib):
    U.check_dsgplus(emu_lib)


def test_guidance_and_variant5_twins_hold(emu_lib):
    U.check_guided_v5(emu_lib)


def test_lanes_2x2_1x4_4x1(emu_lib):
    U.check_lanes(emu_lib)


def test_raw_export_state_and_refusals(emu_lib):
    U.check_raw_and_state(emu_lib)


def test_plan_steps(emu_lib):
    U.check_plan(emu_lib)


def test_abi(emu_lib):
    U.check_abi(emu_lib)
