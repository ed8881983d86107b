"""MI355X: how a step loop is started and run is the call's own -- nothing of it is parked on the handle -- on the product library: the checks
of tests/run_mode_util.py."""
import pytest

from diffusestylegesture_amd import lib as L
from tests import run_mode_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return L.DSGLibrary(hip_lib_path)


def test_refused_clip_call_leaves_nothing_behind(lib):
    U.check_refused_clip_call(lib)


def test_one_shot_queue_call_leaves_nothing_behind(lib):
    U.check_after_queue_call(lib)


def test_closed_session_leaves_nothing_behind(lib):
    U.check_after_session(lib)


def test_user_inpainting_survives_other_calls(lib):
    U.check_user_state_survives(lib)
