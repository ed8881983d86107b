"""MI355X: live jobs of a queue session (dsg_queue_submit_live / _append / _finish) on the product library -- the checks of
tests/clip_queue_live_util.py, plus what only the hardware has: the ROWS set at the ZEGGS widths with a live job that sits a round out, and
every pointer of submit_live / append as a device tensor one float past a 16-byte boundary.  A clip fed window by window must come out bit
for bit as dsg_sample_clip produces those windows alone on a batch-1 handle under the same named kernel set."""
import pytest

from diffusestylegesture_amd import lib as L
from tests import clip_queue_live_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return L.DSGLibrary(hip_lib_path)


def test_live_equals_alone(lib):
    U.check_live_equals_alone(lib)


def test_sitting_out_odd_and_even_rounds(lib):
    U.check_sitting_out(lib)


def test_nothing_to_run(lib):
    U.check_nothing_to_run(lib)


def test_finish_after_the_last_window_ran(lib):
    U.check_finish_late(lib)


def test_finish_early_and_late_keep_last_tail(lib):
    U.check_finish_keep_last_tail(lib)


def test_window_style_and_scale_guided(lib):
    U.check_window_style_scale(lib)


def test_window_style_unguided(lib):
    U.check_window_style(lib)


def test_slots(lib):
    U.check_slots(lib)


def test_lanes_2x1_1x2(lib):
    U.check_lanes(lib)


def test_inputs_are_free_after_append(lib):
    U.check_inputs_free(lib)


def test_refusals(lib):
    U.check_refusals(lib)


def test_abi(lib):
    U.check_abi(lib)


def test_drivers(lib):
    U.check_drivers(lib)


def test_zeggs_widths_rows_set_live_job_sits_out(lib):
    U.check_zeggs_rows(lib)


def test_device_pointers_off_16_bytes(lib):
    U.check_device_pointers(lib)
