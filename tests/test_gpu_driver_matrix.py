"""MI355X: the clip drivers of sample.py with their options together on the product library -- the checks of tests/driver_matrix_util.py
(host == library == alone, bit for bit).  The torch clips of the queue case are device tensors here."""
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from tests import driver_matrix_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return L.DSGLibrary(hip_lib_path)


def test_zeggs_two_lanes_all_options(lib):
    U.check_lanes(lib, C.TINY, 3)


def test_zeggs_single_lane_all_options(lib):
    U.check_single(lib, C.TINY, 3)


def test_dsgpp_two_lanes_all_options(lib):
    U.check_lanes(lib, C.TINY5, 2)


def test_dsgpp_single_lane_all_options(lib):
    U.check_single(lib, C.TINY5, 2, alone=True)


def test_attention3_left_context(lib):
    U.check_single(lib, C.TINY3B, 2)


@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_ddim_init_motion(lib, cfg):
    U.check_ddim(lib, cfg)


def test_custom_sample_fn_keywords(lib):
    U.check_sample_fn(lib)


def test_queue_job_builder(lib):
    U.check_queue_jobs(lib, device="cuda")
