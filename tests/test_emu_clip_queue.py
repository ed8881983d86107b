"""CPU: the clip queue (dsg_clip_queue_plan / dsg_sample_clip_queue, `DSGDiffusion.sample_clip_queue`, `sample.generate_clip_queue[_dsgplus]`)
through the product sources under the SIMT emulator.  Clips of different lengths share one batch of slots; a slot takes the next clip when
its clip ends.  Every clip must come out bit for bit as dsg_sample_clip produces it alone on a batch-1 handle with its own (seed, stream
id), under the same named kernel set.  The checks themselves are tests/clip_queue_util.py; the real-hardware run is
tests/test_gpu_clip_queue.py (-m gpu)."""
import pytest

from diffusestylegesture_amd import config as C
from tests import clip_queue_util as U


def test_plan_reference_values_and_invariants(emu_lib):
    U.check_plan(emu_lib)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_each_clip_equals_the_clip_alone_every_kernel_set(emu_lib, prec):
    """TINY, K = (1, 3, 2, 1, 2) over one lane of B = 2, under every kernel set the handle accepts for batch 2 and batch 1: DDPM with the
    root shift, DDIM (eta 0.5) without; the remaining two combinations under TILE.  skip_timesteps = 996 runs q_sample in the start kernel,
    so the draw offset there is covered by every case (see U.check_each_clip_alone)."""
    sets = U.accepted_sets(emu_lib, C.TINY, prec, 2)
    assert "tile" in sets and len(sets) >= 3, sets
    for ks in sets:
        U.check_each_clip_alone(emu_lib, C.TINY, prec, ks)
    U.check_each_clip_alone(emu_lib, C.TINY, prec, "tile", combos=((False, False), (True, True)))


def test_each_clip_equals_the_clip_alone_bf16w2_tile(emu_lib):
    U.check_each_clip_alone(emu_lib, C.TINY, "bf16w2", "tile")


def test_dsgplus_stitching_keep_last_tail(emu_lib):
    U.check_dsgplus(emu_lib)


def test_guidance_and_variant5(emu_lib):
    U.check_guided_v5(emu_lib)


def test_lanes_2x2_1x4_4x1(emu_lib):
    U.check_lanes(emu_lib)


def test_more_slots_than_clips_and_order(emu_lib):
    U.check_more_slots_and_order(emu_lib)


def test_nothing_sticks(emu_lib):
    U.check_nothing_sticks(emu_lib)


def test_errors(emu_lib):
    U.check_errors(emu_lib)
