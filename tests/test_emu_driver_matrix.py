"""CPU: the clip drivers of sample.py with their options together (`clip_ids` + a constraint + an init motion + a seed pose, a second lane,
a lane whose per-lane entries are None; the queue job builder through the one-shot call, a session and a live clip) through the product
sources under the SIMT emulator.  host == library == alone, bit for bit; the checks themselves are tests/driver_matrix_util.py, the
real-hardware run is tests/test_gpu_driver_matrix.py (-m gpu)."""
import pytest

from diffusestylegesture_amd import config as C
from tests import driver_matrix_util as U


def test_zeggs_two_lanes_all_options(emu_lib):
    U.check_lanes(emu_lib, C.TINY, 3)


def test_zeggs_single_lane_all_options(emu_lib):
    U.check_single(emu_lib, C.TINY, 3)


def test_dsgpp_two_lanes_all_options(emu_lib):
    U.check_lanes(emu_lib, C.TINY5, 2)


def test_dsgpp_single_lane_all_options(emu_lib):
    U.check_single(emu_lib, C.TINY5, 2, alone=True)


def test_attention3_left_context(emu_lib):
    U.check_single(emu_lib, C.TINY3B, 2)


@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_ddim_init_motion(emu_lib, cfg):
    U.check_ddim(emu_lib, cfg)


def test_custom_sample_fn_keywords(emu_lib):
    U.check_sample_fn(emu_lib)


def test_queue_job_builder(emu_lib):
    U.check_queue_jobs(emu_lib)
