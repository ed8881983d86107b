"""CPU: what a handle reports about its last sampling call (dsg_last_sample_ms / _path / _fence_free, dsg_last_kernel_set) is one report,
committed once where the call succeeds -- through the product sources under the SIMT emulator.  The checks themselves are
tests/last_report_util.py; the real-hardware run, with the assertions on the milliseconds, is tests/test_gpu_last_report.py (-m gpu)."""
from tests import last_report_util as U


def test_fresh_handle_and_forward(emu_lib):
    U.check_fresh_and_forward(emu_lib)


def test_sample_reports_its_steps(emu_lib):
    U.check_sample(emu_lib)


def test_multi_reports_per_lane(emu_lib):
    U.check_multi(emu_lib)


def test_clip_reports_all_windows(emu_lib):
    U.check_clip(emu_lib)


def test_one_shot_queue_reports_round_lengths(emu_lib):
    U.check_queue(emu_lib)


def test_refused_call_leaves_the_report(emu_lib):
    U.check_refused(emu_lib)


def test_empty_session_run_leaves_the_report(emu_lib):
    U.check_empty_session_run(emu_lib)


def test_session_reports_its_rounds(emu_lib):
    U.check_session(emu_lib)
