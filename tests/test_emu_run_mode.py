"""CPU: how a step loop is started and run is the call's own -- nothing of it is parked on the handle -- through the product sources under the
SIMT emulator.  A refused whole-clip call, a one-shot queue call and a closed queue session each leave a handle that samples what a fresh
clone samples; dsg_set_inpainting survives whole-clip and multi-lane calls.  The checks themselves are tests/run_mode_util.py; the
real-hardware run is tests/test_gpu_run_mode.py (-m gpu)."""
from tests import run_mode_util as U


def test_refused_clip_call_leaves_nothing_behind(emu_lib):
    U.check_refused_clip_call(emu_lib)


def test_one_shot_queue_call_leaves_nothing_behind(emu_lib):
    U.check_after_queue_call(emu_lib)


def test_closed_session_leaves_nothing_behind(emu_lib):
    U.check_after_session(emu_lib)


def test_user_inpainting_survives_other_calls(emu_lib):
    U.check_user_state_survives(emu_lib)
