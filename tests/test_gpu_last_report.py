"""MI355X: what a handle reports about its last sampling call is one report, committed once where the call succeeds -- on the product
library: the checks of tests/last_report_util.py, and on the milliseconds what only real hardware shows."""
import pytest

from diffusestylegesture_amd import lib as L
from tests import last_report_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return L.DSGLibrary(hip_lib_path)


def test_fresh_handle_and_forward(lib):
    U.check_fresh_and_forward(lib)


def test_sample_reports_its_steps(lib):
    ms = U.check_sample(lib)[0]
    print("dsg_sample ms", ms)
    assert ms > 0


def test_multi_reports_per_lane(lib):
    U.check_multi(lib)


def test_clip_reports_all_windows(lib):
    clip, one = U.check_clip(lib)
    print("dsg_sample_clip ms", clip[0], "dsg_sample ms", one[0])
    assert clip[0] > 0 and clip[0] >= one[0]                  # two windows cannot take less than one


def test_one_shot_queue_reports_round_lengths(lib):
    U.check_queue(lib)


def test_refused_call_leaves_the_report(lib):
    U.check_refused(lib)


def test_empty_session_run_leaves_the_report(lib):
    U.check_empty_session_run(lib)


def test_session_reports_its_rounds(lib):
    ms = U.check_session(lib)[0]
    print("session ms", ms)
    assert ms > 0
