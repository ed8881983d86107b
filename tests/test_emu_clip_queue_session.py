"""CPU: the clip queue as a session (dsg_queue_open / _submit / _run / _job / _info / _cancel / _close and dsg_queue_place;
`DSGDiffusion.open_clip_queue`, `sample.open_clip_queue[_dsgplus]`) through the product sources under the SIMT emulator.  Clips are submitted
while the session runs and collected window by window; every clip must come out bit for bit as dsg_sample_clip produces it alone on a batch-1
handle, under the same named kernel set, whenever it was submitted and whatever was cancelled beside it.  The checks themselves are
tests/clip_queue_session_util.py; the real-hardware run is tests/test_gpu_clip_queue_session.py (-m gpu)."""
import pytest

from diffusestylegesture_amd import config as C
from tests import clip_queue_session_util as U


def test_place(emu_lib):
    U.check_place(emu_lib)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_arrivals_every_kernel_set(emu_lib, prec):
    """TINY, one lane of B = 2, K = (3, 1, 2, 1, 2) submitted before rounds (0, 0, 1, 1, 2), under every kernel set the handle accepts for
    batch 2 and batch 1: DDPM with the root shift and DDIM (eta 0.5) without; dsg_queue_job reports the issue's table round by round"""
    sets = U.accepted_sets(emu_lib, C.TINY, prec, 2)
    assert "tile" in sets and len(sets) >= 3, sets
    for ks in sets:
        U.check_arrivals(emu_lib, C.TINY, prec, ks)


def test_delivery_per_window(emu_lib):
    U.check_delivery(emu_lib, C.TINY, False)


def test_delivery_per_window_keep_last_tail(emu_lib):
    U.check_delivery(emu_lib, C.TINY4, True)


def test_inputs_are_free_after_submit(emu_lib):
    U.check_inputs_free(emu_lib)


def test_edits_and_strengths_arriving_late(emu_lib):
    U.check_late_edits(emu_lib)


def test_cancel(emu_lib):
    U.check_cancel(emu_lib)


def test_lanes_2x2_1x4_4x1(emu_lib):
    U.check_lanes(emu_lib)


def test_guidance_and_variant5_dsgplus_driver(emu_lib):
    U.check_guided_v5(emu_lib)


def test_zeggs_driver_holds_the_kernel_set(emu_lib):
    U.check_zeggs_driver(emu_lib)


def test_ownership_and_nothing_sticks(emu_lib):
    U.check_ownership(emu_lib)


def test_open_and_submit_refusals(emu_lib):
    U.check_open_refusals(emu_lib)


def test_abi(emu_lib):
    U.check_abi(emu_lib)
