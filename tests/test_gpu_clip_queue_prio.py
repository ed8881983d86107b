"""MI355X: job priorities, park and resume in a queue session (dsg_queue_set_priority / _park / _resume / dsg_queue_place_prio) on the
product library -- the checks of tests/clip_queue_prio_util.py, plus what only the hardware has: pre-emption in the ROWS set at the ZEGGS
widths, the two tail buffers at the BEAT++ widths (variant 5), and every job tensor as a device tensor one float past a 16-byte boundary.
A job that was parked and resumed must come out bit for bit as dsg_sample_clip produces it alone on a batch-1 handle under the same named
kernel set."""
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from tests import clip_queue_prio_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return L.DSGLibrary(hip_lib_path)


def test_order_by_priority_then_ticket(lib):
    U.check_order(lib)


def test_preemption_parks_and_resumes(lib):
    U.check_preempt(lib)


def test_tail_parity_odd_and_even_resume_in_the_other_slot(lib):
    U.check_tail_parity(lib)


def test_tail_parity_dsgplus_variant5_seed_last_follows(lib):
    U.check_tail_parity(lib, C.TINY5)


def test_equal_priorities_change_nothing(lib):
    U.check_equal_priorities(lib)


def test_explicit_park_and_resume(lib):
    U.check_park_resume(lib)


def test_idle_live_job_is_the_first_victim(lib):
    U.check_live_victim(lib)


def test_finish_on_a_parked_live_job_keep_last_tail(lib):
    U.check_live_finish_parked(lib)


def test_finish_on_a_parked_live_job_zeggs_layout(lib):
    U.check_live_finish_parked(lib, C.TINY)


def test_lanes_park_on_lane_0_resume_on_lane_1(lib):
    U.check_lanes(lib)


def test_everything_a_job_carries_root_shift(lib):
    U.check_everything(lib)


def test_everything_a_job_carries_variant5(lib):
    U.check_everything(lib, C.TINY5)


def test_cancel_on_a_parked_job(lib):
    U.check_cancel_parked(lib)


def test_close_with_parked_and_held_jobs(lib):
    U.check_close_parked(lib)


def test_refusals(lib):
    U.check_refusals(lib)


def test_host_plan(lib):
    U.check_place_prio(lib)


def test_abi(lib):
    U.check_abi(lib)


def test_drivers(lib):
    U.check_drivers(lib)


def test_zeggs_widths_rows_set_preemption(lib):
    U.check_zeggs_rows(lib)


def test_beatpp_widths_rows_set_tail_parity_variant5(lib):
    U.check_beatpp_rows(lib)


def test_device_pointers_off_16_bytes(lib):
    U.check_device_pointers(lib)
