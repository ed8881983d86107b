"""CPU: job priorities, park and resume in a queue session (dsg_queue_set_priority / _park / _resume / dsg_queue_place_prio; `ClipQueue`
and the two drivers of sample.py) through the product sources under the SIMT emulator.  A job that leaves its slot at a window boundary --
pre-empted by a higher priority or parked by the caller -- and continues later in any slot of any lane must come out bit for bit as
dsg_sample_clip produces it alone on a batch-1 handle, under the same named kernel set.  The checks themselves are
tests/clip_queue_prio_util.py; the real-hardware run is tests/test_gpu_clip_queue_prio.py (-m gpu)."""
from diffusestylegesture_amd import config as C
from tests import clip_queue_prio_util as U


def test_order_by_priority_then_ticket(emu_lib):
    U.check_order(emu_lib)


def test_preemption_parks_and_resumes(emu_lib):
    U.check_preempt(emu_lib)


def test_tail_parity_odd_and_even_resume_in_the_other_slot(emu_lib):
    U.check_tail_parity(emu_lib)


def test_tail_parity_dsgplus_variant5_seed_last_follows(emu_lib):
    U.check_tail_parity(emu_lib, C.TINY5, afters=(1,))


def test_equal_priorities_change_nothing(emu_lib):
    U.check_equal_priorities(emu_lib)


def test_explicit_park_and_resume(emu_lib):
    U.check_park_resume(emu_lib)


def test_idle_live_job_is_the_first_victim(emu_lib):
    U.check_live_victim(emu_lib)


def test_finish_on_a_parked_live_job_keep_last_tail(emu_lib):
    U.check_live_finish_parked(emu_lib)


def test_finish_on_a_parked_live_job_zeggs_layout(emu_lib):
    U.check_live_finish_parked(emu_lib, C.TINY)


def test_lanes_park_on_lane_0_resume_on_lane_1(emu_lib):
    U.check_lanes(emu_lib)


def test_everything_a_job_carries_root_shift(emu_lib):
    U.check_everything(emu_lib)


def test_everything_a_job_carries_variant5(emu_lib):
    U.check_everything(emu_lib, C.TINY5)


def test_cancel_on_a_parked_job(emu_lib):
    U.check_cancel_parked(emu_lib)


def test_close_with_parked_and_held_jobs(emu_lib):
    U.check_close_parked(emu_lib)


def test_refusals(emu_lib):
    U.check_refusals(emu_lib)


def test_host_plan(emu_lib):
    U.check_place_prio(emu_lib)


def test_abi(emu_lib):
    U.check_abi(emu_lib)


def test_drivers(emu_lib):
    U.check_drivers(emu_lib)
