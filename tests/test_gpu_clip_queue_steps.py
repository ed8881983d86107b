"""MI355X (-m gpu): per-clip skip_timesteps in the clip queue (dsg_sample_clip_queue_steps) on the real kernels -- the checks of
tests/clip_queue_steps_util.py, which the emulator runs in tests/test_emu_clip_queue_steps.py, plus what only exists here: device pointers,
the streaming pose head k_ws<EPI_OUT> of the ROWS set at the ZEGGS widths and its guided form k_ws_cfg at the BEAT width.  One kernel set is
named for both sides of every comparison."""
import pytest

from diffusestylegesture_amd import config as C
from tests import clip_queue_steps_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mixed_strengths_every_kernel_set(gpu, prec):
    """as the emulator twin"""
    sets = U.accepted_sets(gpu, C.TINY, prec, 2)
    print("kernel sets:", sets)
    assert "tile" in sets
    for ks in sets:
        U.check_mixed(gpu, C.TINY, prec, ks)
    U.check_mixed(gpu, C.TINY, prec, "tile", cases=U.CROSS)


def test_mixed_strengths_bf16w2_tile(gpu):
    U.check_mixed(gpu, C.TINY, "bf16w2", "tile")


def test_deep_holds_and_ddim_eta_0(gpu):
    U.check_deep_holds(gpu)


def test_fresh_beside_edits_four_step_schedule(gpu):
    U.check_fresh_beside_edits(gpu)


def test_dsgplus_stitching_keep_last_tail(gpu):
    U.check_dsgplus(gpu)


def test_guidance_and_variant5_twins_hold(gpu):
    U.check_guided_v5(gpu)


def test_lanes_2x2_1x4_4x1(gpu):
    U.check_lanes(gpu)


def test_raw_export_state_and_refusals(gpu):
    U.check_raw_and_state(gpu)


def test_device_pointers(gpu):
    U.check_device_pointers(gpu)


def test_plan_steps(gpu):
    U.check_plan(gpu)


def test_product_widths_zeggs_rows(gpu):
    """ZEGGS, bf16, ROWS named, K = (2, 1, 1, 1) over B = 3, skips (996, 998, 994, 999): job 0 with constraint and init"""
    U.check_zeggs_rows(gpu)


def test_product_widths_beat_rows_guided(gpu):
    """BEAT width (variant 5), bf16, ROWS named, guided: two K = 1 jobs, B = 2 plus twins, skips (998, 996)"""
    U.check_beat_rows_guided(gpu)


def test_abi(gpu):
    U.check_abi(gpu)
