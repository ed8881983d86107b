"""CPU: per-clip inpainting and init motion in the clip queue (dsg_sample_clip_queue_edit; the "inpainting_mask" / "inpainted_motion" /
"init_motion" keys of `DSGDiffusion.sample_clip_queue` and `sample.generate_clip_queue[_dsgplus]`) through the product sources under the SIMT
emulator.  Every clip must come out bit for bit as dsg_sample_clip produces it alone on a batch-1 handle after dsg_set_clip_inpainting /
dsg_set_clip_init with its own edits, under the same named kernel set; a clip without edits as it does alone without.  The checks themselves
are tests/clip_queue_edit_util.py; the real-hardware run is tests/test_gpu_clip_queue_edit.py (-m gpu)."""
import pytest

from diffusestylegesture_amd import config as C
from tests import clip_queue_edit_util as U


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mixed_queue_every_kernel_set(emu_lib, prec):
    """TINY, K = (1, 3, 2, 1, 2) over one lane of B = 2, under every kernel set the handle accepts for batch 2 and batch 1: assignment A of
    edits to jobs under DDPM with the root shift, assignment B under DDIM (eta 0.5) without; the other pairing under TILE"""
    sets = U.accepted_sets(emu_lib, C.TINY, prec, 2)
    assert "tile" in sets and len(sets) >= 3, sets
    for ks in sets:
        U.check_mixed(emu_lib, C.TINY, prec, ks)
    U.check_mixed(emu_lib, C.TINY, prec, "tile", cases=U.CROSS)


def test_mixed_queue_bf16w2_tile(emu_lib):
    U.check_mixed(emu_lib, C.TINY, "bf16w2", "tile")


def test_skip_timesteps_0_init_beside_plain(emu_lib):
    U.check_skip0(emu_lib)


def test_dsgplus_stitching_keep_last_tail(emu_lib):
    U.check_dsgplus(emu_lib)


def test_guidance_and_variant5(emu_lib):
    U.check_guided_v5(emu_lib)


def test_lanes_2x2_1x4_4x1(emu_lib):
    U.check_lanes(emu_lib)


def test_raw_export_nothing_sticks_and_errors(emu_lib):
    U.check_raw_and_state(emu_lib)


def test_abi(emu_lib):
    U.check_abi(emu_lib)
