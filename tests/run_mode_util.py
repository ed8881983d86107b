"""Shared by tests/test_emu_run_mode.py (CPU, the SIMT emulator) and tests/test_gpu_run_mode.py (MI355X): a sampling call leaves nothing of
its own mode on the handle -- not the lane count, not the start kernel, not the epilogue's inpainting, not a key table -- and takes nothing of
the user's sticky state (dsg_set_inpainting) away.  Everything that changes or reads a handle's state goes through the C ABI
(`DSGLibrary.cdll`); every comparison is `np.array_equal` against the same dsg_sample on a clone that never saw the call in question.  TINY,
bf16, AUTO kernel set, a respaced schedule of four steps, clips of K = 2 windows."""
import ctypes

import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from tests.clip_queue_edit_util import BOTH, diffusion_4, edit_of
from tests.clip_queue_session_util import RawSession
from tests.clip_queue_util import PAIRS, clip_of, model, n_out_of, y_of

CFG, PREC, K = C.TINY, "bf16", 2
JOB_SKIP = 1                           # the edited clip's own skip_timesteps: three of the four steps


def _args(skip=0):
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps, a.seed, a.stream_id = L.MODE_DDPM, skip, 5, 3
    return a


def _lane(lib, d, B, of=None):
    m = model(lib, CFG, PREC, B) if of is None else of.clone(B)
    m.set_schedule(d)
    return m


def sample(lib, m, B=1):
    """dsg_sample at batch B on the window conditioning of clips 10, 11: [B, J, 1, T]"""
    m.set_cond(y_of(CFG, (10, 11)[:B]), B)
    out = np.zeros((B, CFG.njoints, 1, CFG.n_poses), np.float32)
    lib.check(lib.cdll.dsg_sample(m.handle, ctypes.byref(_args()), out.ctypes.data, B, None))
    return out


def last_set(lib, m):
    s = ctypes.c_int(-1)
    lib.check(lib.cdll.dsg_last_kernel_set(m.handle, ctypes.byref(s)))
    return s.value


def single_lane_set(lib, m, B=1):
    s = ctypes.c_int(-1)
    lib.check(lib.cdll.dsg_recommend_kernel_set(m.handle, B, 1, ctypes.byref(s)))
    return s.value


def _edited_clip():
    """one clip with a mask, an init motion and (the callers) its own skip: the clip, its Philox pair, its edits [n_out, J]"""
    return clip_of(CFG, 20, K), PAIRS[0], edit_of(CFG, K, False, 0, BOTH)


def _same_as_fresh(lib, d, m, B=1):
    """dsg_sample on m equals dsg_sample on a clone made now, under the kernel set AUTO picks for one lane"""
    fresh = _lane(lib, d, B, of=m)
    got, want = sample(lib, m, B), sample(lib, fresh, B)
    assert np.isfinite(want).all() and np.array_equal(got, want), float(np.max(np.abs(got - want)))
    assert last_set(lib, m) == last_set(lib, fresh) == single_lane_set(lib, m, B)


# ---- 1. a refused whole-clip call leaves nothing behind ------------------------------------------------------------------------------------
def check_refused_clip_call(lib):
    d = diffusion_4(lib)
    m = _lane(lib, d, 2)
    h, cd = m.handle, lib.cdll
    clip, _, edit = _edited_clip()
    n_out = n_out_of(CFG, K, False)
    mask, motion, init = edit["inpainting_mask"][None], edit["inpainted_motion"][None], edit["init_motion"][None]
    streams = np.array([7, 9], np.uint64)
    lib.check(cd.dsg_set_clip_inpainting(h, mask.ctypes.data, motion.ctypes.data, 1, n_out, None))
    lib.check(cd.dsg_set_clip_init(h, init.ctypes.data, 1, n_out, None))
    lib.check(cd.dsg_set_noise_streams(h, None, streams.ctypes.data, 2))
    audio = np.ascontiguousarray(np.concatenate(clip["feats"]), np.float32)
    out = np.zeros((1, n_out, CFG.njoints), np.float32)
    ones = np.ones(CFG.n_poses, np.uint8)
    # the noise-stream batch (2) against the call's (1): refused inside window 0, behind the cut of its constraint and the choice of its start
    rc = cd.dsg_sample_clip(h, clip["style"].ctypes.data, clip["seed"].ctypes.data, audio.ctypes.data, ones.ctypes.data, 1, None,
                            ctypes.byref(_args()), K, 1, 0, out.ctypes.data, 1, None)
    assert rc == L.E_INVALID and b"batch 1 differs from the batch of dsg_set_noise_streams (2)" in cd.dsg_last_error()
    lib.check(cd.dsg_set_clip_inpainting(h, None, None, 0, 0, None))
    lib.check(cd.dsg_set_clip_init(h, None, 0, 0, None))
    lib.check(cd.dsg_set_noise_streams(h, None, None, 0))
    _same_as_fresh(lib, d, m)


# ---- 2. the same after a one-shot queue call and after a closed session ---------------------------------------------------------------------
def check_after_queue_call(lib):
    """two lanes of B = 1: lane 0 runs the edited clip (constraint cut every round, start through the edit table, a keyed table with draw
    offsets), lane 1 a dead slot"""
    d = diffusion_4(lib)
    m = _lane(lib, d, 1)
    lanes = [m, _lane(lib, d, 1, of=m)]
    clip, (seed, sid), edit = _edited_clip()
    audio = np.ascontiguousarray(np.concatenate(clip["feats"]), np.float32)
    out = np.zeros((n_out_of(CFG, K, False), CFG.njoints), np.float32)
    job, ed = L.dsg_clip_job(), L.dsg_clip_edit()
    job.style, job.seed0, job.audio, job.out = clip["style"].ctypes.data, clip["seed"].ctypes.data, audio.ctypes.data, out.ctypes.data
    job.K, job.scale, job.seed, job.stream_id = K, 1.0, seed, sid
    ed.inp_mask, ed.inp_motion, ed.init_motion = (edit[k].ctypes.data for k in ("inpainting_mask", "inpainted_motion", "init_motion"))
    skips = np.array([JOB_SKIP], np.int32)
    hs = (ctypes.c_void_p * 2)(*[ln.handle for ln in lanes])
    ones = np.ones(CFG.n_poses, np.uint8)
    lib.check(lib.cdll.dsg_sample_clip_queue_steps(hs, 2, ctypes.byref(job), ctypes.byref(ed), skips.ctypes.data, 1, 1, ones.ctypes.data, 0,
                                                   ctypes.byref(_args()), 1, 0, None))
    assert np.isfinite(out).all() and out.any()
    for ln in lanes:
        _same_as_fresh(lib, d, ln)


def check_after_session(lib):
    d = diffusion_4(lib)
    m = _lane(lib, d, 1)
    lanes = [m, _lane(lib, d, 1, of=m)]
    clip, pair, edit = _edited_clip()
    s = RawSession(lib, [ln.handle for ln in lanes], CFG, 1, skip=0)
    assert s.rc == 0, s.msg
    try:
        t = s.submit(clip, pair, edit, skip=JOB_SKIP)
        assert s.run(0) == K
        got = s.out(t)
        assert np.isfinite(got).all() and got[:-2].any()
    finally:
        s.close()
    for ln in lanes:
        _same_as_fresh(lib, d, ln)


# ---- 3. the user's state survives ---------------------------------------------------------------------------------------------------------
def check_user_state_survives(lib):
    d = diffusion_4(lib)
    a = _lane(lib, d, 1)
    b = _lane(lib, d, 1, of=a)
    cd = lib.cdll
    shape = (1, CFG.njoints, 1, CFG.n_poses)
    mask = np.zeros(shape, np.uint8)
    mask[:, 3::3, :, 5:20] = 1
    motion = (0.5 * np.random.default_rng(3).standard_normal(shape)).astype(np.float32)
    plain = sample(lib, a)
    lib.check(cd.dsg_set_inpainting(a.handle, mask.ctypes.data, motion.ctypes.data, 1, None))
    before = sample(lib, a)
    mk = mask != 0
    assert np.array_equal(before[mk], motion[mk]) and not np.array_equal(before, plain)      # (the last step's posterior mean is x0 itself)
    # a whole-clip call on another lane of the model ...
    clip = clip_of(CFG, 20, K)
    audio = np.ascontiguousarray(np.concatenate(clip["feats"]), np.float32)
    out = np.zeros((1, n_out_of(CFG, K, False), CFG.njoints), np.float32)
    ones = np.ones(CFG.n_poses, np.uint8)
    lib.check(cd.dsg_sample_clip(b.handle, clip["style"].ctypes.data, clip["seed"].ctypes.data, audio.ctypes.data, ones.ctypes.data, 1, None,
                                 ctypes.byref(_args()), K, 1, 0, out.ctypes.data, 1, None))
    # ... and a dsg_sample_multi over both: lane a inpainted, lane b not
    for ln in (a, b):
        ln.set_cond(y_of(CFG, (10,)), 1)
    outs = [np.zeros(shape, np.float32) for _ in range(2)]
    hs = (ctypes.c_void_p * 2)(a.handle, b.handle)
    args = (L.dsg_sample_args * 2)(_args(), _args())
    ptrs = (ctypes.c_void_p * 2)(*[o.ctypes.data for o in outs])
    lib.check(cd.dsg_sample_multi(hs, 2, args, ptrs, 1, None))
    assert np.array_equal(outs[0], before) and np.array_equal(outs[1], plain)
    assert np.array_equal(sample(lib, a), before)
    lib.check(cd.dsg_set_inpainting(a.handle, None, None, 0, None))
    assert np.array_equal(sample(lib, a), plain)
