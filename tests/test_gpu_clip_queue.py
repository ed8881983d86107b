"""MI355X (-m gpu): the clip queue (dsg_clip_queue_plan / dsg_sample_clip_queue) on the real kernels -- the checks of
tests/clip_queue_util.py, which the emulator runs in tests/test_emu_clip_queue.py, plus what only exists here: the streaming pose head
k_ws<EPI_OUT> of the ROWS set at the ZEGGS widths.  One kernel set is named for both sides of every comparison."""
import pytest

from diffusestylegesture_amd import config as C
from tests import clip_queue_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_each_clip_equals_the_clip_alone_every_kernel_set(gpu, prec):
    """as the emulator twin; skip_timesteps = 996 runs q_sample in the start kernel, so the draw offset there is covered by every case"""
    sets = U.accepted_sets(gpu, C.TINY, prec, 2)
    print("kernel sets:", sets)
    assert "tile" in sets
    for ks in sets:
        U.check_each_clip_alone(gpu, C.TINY, prec, ks)
    U.check_each_clip_alone(gpu, C.TINY, prec, "tile", combos=((False, False), (True, True)))


def test_each_clip_equals_the_clip_alone_bf16w2_tile(gpu):
    U.check_each_clip_alone(gpu, C.TINY, "bf16w2", "tile")


def test_dsgplus_stitching_keep_last_tail(gpu):
    U.check_dsgplus(gpu)


def test_guidance_and_variant5(gpu):
    U.check_guided_v5(gpu)


def test_lanes_2x2_1x4_4x1(gpu):
    U.check_lanes(gpu)


def test_more_slots_than_clips_and_order(gpu):
    U.check_more_slots_and_order(gpu)


def test_nothing_sticks(gpu):
    U.check_nothing_sticks(gpu)


def test_errors(gpu):
    U.check_errors(gpu)


def test_product_widths_zeggs_rows(gpu):
    """ZEGGS, bf16, ROWS named, K = (2, 1, 1, 1) over B = 3, four steps: each clip against the batch-1 clip alone"""
    U.check_zeggs_rows(gpu)


def test_device_pointers_write_the_callers_out(gpu):
    U.check_device_pointers(gpu)
