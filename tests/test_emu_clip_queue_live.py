"""CPU: live jobs of a queue session (dsg_queue_submit_live / _append / _finish; `ClipQueue.submit_live` / `append` / `finish` and the two
drivers of sample.py) through the product sources under the SIMT emulator.  A clip whose windows arrive while it runs must come out bit for
bit as dsg_sample_clip produces those windows alone on a batch-1 handle, under the same named kernel set -- whenever the windows arrived,
however many rounds the job sat out, whatever ran beside it.  The checks themselves are tests/clip_queue_live_util.py; the real-hardware run
is tests/test_gpu_clip_queue_live.py (-m gpu)."""
from tests import clip_queue_live_util as U


def test_live_equals_alone(emu_lib):
    U.check_live_equals_alone(emu_lib)


def test_sitting_out_odd_and_even_rounds(emu_lib):
    """the one that fails on a hand-off that picks the tail buffers by the session's round"""
    U.check_sitting_out(emu_lib)


def test_nothing_to_run(emu_lib):
    U.check_nothing_to_run(emu_lib)


def test_finish_after_the_last_window_ran(emu_lib):
    U.check_finish_late(emu_lib)


def test_finish_early_and_late_keep_last_tail(emu_lib):
    U.check_finish_keep_last_tail(emu_lib)


def test_window_style_and_scale_guided(emu_lib):
    U.check_window_style_scale(emu_lib)


def test_window_style_unguided(emu_lib):
    U.check_window_style(emu_lib)


def test_slots(emu_lib):
    U.check_slots(emu_lib)


def test_lanes_2x1_1x2(emu_lib):
    U.check_lanes(emu_lib)


def test_inputs_are_free_after_append(emu_lib):
    U.check_inputs_free(emu_lib)


def test_refusals(emu_lib):
    U.check_refusals(emu_lib)


def test_abi(emu_lib):
    U.check_abi(emu_lib)


def test_drivers(emu_lib):
    U.check_drivers(emu_lib)
