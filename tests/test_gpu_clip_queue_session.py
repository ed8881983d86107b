"""MI355X: the clip queue as a session (dsg_queue_*; `DSGDiffusion.open_clip_queue`, `sample.open_clip_queue[_dsgplus]`) on the product
library -- the checks of tests/clip_queue_session_util.py, plus what only the hardware has: the ROWS set at the ZEGGS widths and every job
pointer as a device tensor one float past a 16-byte boundary (the 4-byte path of k_clipq_gather beside its 16-byte path).  Every clip must
come out bit for bit as dsg_sample_clip produces it alone on a batch-1 handle under the same named kernel set."""
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from tests import clip_queue_session_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return L.DSGLibrary(hip_lib_path)


def test_place(lib):
    U.check_place(lib)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_arrivals_every_kernel_set(lib, prec):
    sets = U.accepted_sets(lib, C.TINY, prec, 2)
    assert "tile" in sets and len(sets) >= 3, sets
    for ks in sets:
        U.check_arrivals(lib, C.TINY, prec, ks)


def test_delivery_per_window(lib):
    U.check_delivery(lib, C.TINY, False)


def test_delivery_per_window_keep_last_tail(lib):
    U.check_delivery(lib, C.TINY4, True)


def test_inputs_are_free_after_submit(lib):
    U.check_inputs_free(lib)


def test_edits_and_strengths_arriving_late(lib):
    U.check_late_edits(lib)


def test_cancel(lib):
    U.check_cancel(lib)


def test_lanes_2x2_1x4_4x1(lib):
    U.check_lanes(lib)


def test_guidance_and_variant5_dsgplus_driver(lib):
    U.check_guided_v5(lib)


def test_zeggs_driver_holds_the_kernel_set(lib):
    U.check_zeggs_driver(lib)


def test_ownership_and_nothing_sticks(lib):
    U.check_ownership(lib)


def test_open_and_submit_refusals(lib):
    U.check_open_refusals(lib)


def test_abi(lib):
    U.check_abi(lib)


def test_zeggs_widths_rows_set(lib):
    U.check_zeggs_rows(lib)


def test_device_pointers_off_16_bytes(lib):
    U.check_device_pointers(lib, C.TINY, False)


def test_device_pointers_off_16_bytes_keep_last_tail(lib):
    U.check_device_pointers(lib, C.TINY4, True)
