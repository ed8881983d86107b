"""Shared by tests/test_emu_last_report.py (CPU, the SIMT emulator) and tests/test_gpu_last_report.py (MI355X): what a handle reports about
its last sampling call -- dsg_last_sample_ms (milliseconds, steps), dsg_last_sample_path, dsg_last_sample_fence_free, dsg_last_kernel_set --
is one report, committed once where the call succeeds.  A fresh handle has none; dsg_forward leaves the kernel set alone; every entry point
reports its own step count; a refused call and a dsg_queue_run without a round leave the previous report whole, milliseconds included.
Through the C ABI only (`DSGLibrary.cdll`).  TINY, bf16, AUTO kernel set, a respaced schedule of four steps, clips of K = 2 windows.  The
check functions return the reports they read, for the assertions on the milliseconds that hold on the GPU only."""
import ctypes

import numpy as np

from diffusestylegesture_amd import lib as L
from tests import clip_queue_steps_util as QS
from tests.clip_queue_edit_util import diffusion_4
from tests.clip_queue_session_util import RawSession
from tests.clip_queue_util import PAIRS, clip_of, clips_of, model, n_out_of, y_of
from tests.run_mode_util import CFG, K, PREC, _args, _lane, sample, single_lane_set

N_SCHED = 4                            # the steps of diffusion_4


def report(lib, m):
    """(ms, steps, path, fence_free, kernel set) as the four exports give them"""
    cd, h = lib.cdll, m.handle
    ms = ctypes.c_float(-1.0)
    n, path, ff, kset = (ctypes.c_int(-1) for _ in range(4))
    lib.check(cd.dsg_last_sample_ms(h, ctypes.byref(ms), ctypes.byref(n)))
    lib.check(cd.dsg_last_sample_path(h, ctypes.byref(path)))
    lib.check(cd.dsg_last_sample_fence_free(h, ctypes.byref(ff)))
    lib.check(cd.dsg_last_kernel_set(h, ctypes.byref(kset)))
    assert path.value in (0, 1, 2) and ff.value in (0, 1) and np.isfinite(ms.value) and ms.value >= 0.0
    return ms.value, n.value, path.value, ff.value, kset.value


def no_sample_report(lib, m):
    """the three dsg_last_sample_* exports refuse: no sampling call has completed on the handle"""
    cd, h = lib.cdll, m.handle
    ms, n = ctypes.c_float(-1.0), ctypes.c_int(-1)
    assert cd.dsg_last_sample_ms(h, ctypes.byref(ms), ctypes.byref(n)) == L.E_STATE
    assert cd.dsg_last_sample_path(h, ctypes.byref(n)) == L.E_STATE
    assert cd.dsg_last_sample_fence_free(h, ctypes.byref(n)) == L.E_STATE


def _sample(lib, m, B=1, **kw):
    """dsg_sample at batch B with fields of dsg_sample_args set from kw"""
    m.set_cond(y_of(CFG, (10, 11)[:B]), B)
    a = _args()
    for k, v in kw.items():
        setattr(a, k, v)
    out = np.zeros((B, CFG.njoints, 1, CFG.n_poses), np.float32)
    lib.check(lib.cdll.dsg_sample(m.handle, ctypes.byref(a), out.ctypes.data, B, None))
    return out


def _clip_call(lib, m, a=None):
    """dsg_sample_clip of one clip of K windows at batch 1: the return code"""
    clip = clip_of(CFG, 20, K)
    audio = np.ascontiguousarray(np.concatenate(clip["feats"]), np.float32)
    out = np.zeros((1, n_out_of(CFG, K, False), CFG.njoints), np.float32)
    ones = np.ones(CFG.n_poses, np.uint8)
    return lib.cdll.dsg_sample_clip(m.handle, clip["style"].ctypes.data, clip["seed"].ctypes.data, audio.ctypes.data, ones.ctypes.data, 1, None,
                                    ctypes.byref(a or _args()), K, 1, 0, out.ctypes.data, 1, None)


def _after_clip(lib, B=2):
    """a lane of max_batch B that has sampled one clip (check 4): (diffusion, lane, its report)"""
    d = diffusion_4(lib)
    m = _lane(lib, d, B)
    lib.check(_clip_call(lib, m))
    return d, m, report(lib, m)


def _empty_session_run(lib, m, B):
    s = RawSession(lib, [m.handle], CFG, B, skip=0)
    assert s.rc == 0, s.msg
    try:
        assert s.run(0) == 0
    finally:
        s.close()


# ---- 1. a fresh handle, and dsg_forward -----------------------------------------------------------------------------------------------------
def check_fresh_and_forward(lib, B=1):
    m = _lane(lib, diffusion_4(lib), B)
    kset = ctypes.c_int(-1)
    no_sample_report(lib, m)
    assert lib.cdll.dsg_last_kernel_set(m.handle, ctypes.byref(kset)) == L.E_STATE
    m.set_cond(y_of(CFG, (10,)), B)
    x = (0.5 * np.random.default_rng(1).standard_normal((B, CFG.njoints, 1, CFG.n_poses))).astype(np.float32)
    t, out = np.array([5] * B, np.int64), np.zeros_like(x)
    lib.check(lib.cdll.dsg_forward(m.handle, x.ctypes.data, t.ctypes.data, out.ctypes.data, B, None))
    assert np.isfinite(out).all() and out.any()
    lib.check(lib.cdll.dsg_last_kernel_set(m.handle, ctypes.byref(kset)))
    assert kset.value == single_lane_set(lib, m, B)
    no_sample_report(lib, m)                                                         # not a sampling call


# ---- 2. dsg_sample ---------------------------------------------------------------------------------------------------------------------------
def check_sample(lib):
    m = _lane(lib, diffusion_4(lib), 1)
    assert np.isfinite(_sample(lib, m)).all()
    first = report(lib, m)
    assert first[1] == N_SCHED and first[4] == single_lane_set(lib, m)
    _sample(lib, m, skip_timesteps=1)
    assert report(lib, m)[1] == N_SCHED - 1
    _sample(lib, m, first_step=0, max_steps=2)
    assert report(lib, m)[1] == 2
    return first


# ---- 3. dsg_sample_multi: every lane its own report --------------------------------------------------------------------------------------------
def check_multi(lib):
    d = diffusion_4(lib)
    a = _lane(lib, d, 1)
    lanes = [a, _lane(lib, d, 1, of=a)]
    for ln in lanes:
        ln.set_cond(y_of(CFG, (10,)), 1)
    outs = [np.zeros((1, CFG.njoints, 1, CFG.n_poses), np.float32) for _ in lanes]
    hs = (ctypes.c_void_p * 2)(*[ln.handle for ln in lanes])
    args = (L.dsg_sample_args * 2)(_args(0), _args(2))
    ptrs = (ctypes.c_void_p * 2)(*[o.ctypes.data for o in outs])
    lib.check(lib.cdll.dsg_sample_multi(hs, 2, args, ptrs, 1, None))
    assert all(np.isfinite(o).all() for o in outs)
    reports = [report(lib, ln) for ln in lanes]
    assert [r[1] for r in reports] == [N_SCHED, N_SCHED - 2]
    return reports


# ---- 4. dsg_sample_clip ---------------------------------------------------------------------------------------------------------------------
def check_clip(lib):
    """returns (the clip's report, the report of one dsg_sample at the same batch on a clone)"""
    d, m, clip = _after_clip(lib, 1)
    assert clip[1] == K * N_SCHED
    fresh = _lane(lib, d, 1, of=m)
    sample(lib, fresh)
    one = report(lib, fresh)
    assert clip[2:] == one[2:]                                                       # path, fence-free, kernel set: as dsg_sample on the same lane
    return clip, one


# ---- 5. the one-shot queue --------------------------------------------------------------------------------------------------------------------
def check_queue(lib, Ks=(2, 1, 2), skips=(0, 1, 0), B=2):
    m = _lane(lib, diffusion_4(lib), B)
    slot, first, n_rounds, total = QS.plan_raw(lib, Ks, B, [N_SCHED - s for s in skips])
    # a round is as long as its deepest job: the schedule less the smallest skip alive in it
    want = sum(N_SCHED - min(skips[j] for j in range(len(Ks)) if first[j] <= r < first[j] + Ks[j]) for r in range(n_rounds))
    assert want == total and n_rounds * (N_SCHED - 1) < want <= n_rounds * N_SCHED   # (the skips matter, and not in every round)
    rc, msg, outs = QS._raw(lib, [m.handle], CFG, clips_of(CFG, Ks), PAIRS[:len(Ks)], None, skips, B, args_skip=0)
    assert rc == 0, msg
    assert all(np.isfinite(o).all() for o in outs)
    got = report(lib, m)
    assert got[1] == want
    return got


# ---- 6. a refused call leaves the report whole --------------------------------------------------------------------------------------------------
def check_refused(lib):
    d, m, before = _after_clip(lib)
    out = np.zeros((2, CFG.njoints, 1, CFG.n_poses), np.float32)
    cd = lib.cdll
    # (the clip left the conditioning of batch 1)
    assert cd.dsg_sample(m.handle, ctypes.byref(_args()), out.ctypes.data, 2, None) == L.E_INVALID
    assert b"batch differs from the batch of dsg_set_window_cond" in cd.dsg_last_error()
    assert report(lib, m) == before
    a = _args()
    a.first_step = 1
    assert _clip_call(lib, m, a) == L.E_INVALID and b"first_step" in cd.dsg_last_error()
    assert report(lib, m) == before


# ---- 7. a session that runs no round leaves the report whole -----------------------------------------------------------------------------------
def check_empty_session_run(lib):
    d, m, before = _after_clip(lib)
    _empty_session_run(lib, m, 2)
    assert report(lib, m) == before


# ---- 8. a session with a job ---------------------------------------------------------------------------------------------------------------------
def check_session(lib, B=2):
    m = _lane(lib, diffusion_4(lib), B)
    s = RawSession(lib, [m.handle], CFG, B, skip=0)
    assert s.rc == 0, s.msg
    try:
        t = s.submit(clip_of(CFG, 20, K), PAIRS[0])
        assert s.run(0) == K
        assert np.isfinite(s.out(t)).all()
    finally:
        s.close()
    got = report(lib, m)
    assert got[1] == K * N_SCHED and got[4] == single_lane_set(lib, m, B)
    _empty_session_run(lib, m, B)
    assert report(lib, m) == got
    return got
