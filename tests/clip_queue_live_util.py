"""Shared by tests/test_emu_clip_queue_live.py (CPU, the SIMT emulator) and tests/test_gpu_clip_queue_live.py (MI355X): the checks of live
jobs in a queue session (dsg_queue_submit_live / _append / _finish; `ClipQueue.submit_live` / `append` / `finish` and the two drivers of
sample.py), written once over a `DSGLibrary`.  Every comparison is `np.array_equal`: a clip fed window by window against the same windows
sampled alone on a batch-1 handle through the existing clip drivers (`windows="library"`) with the same kernel set named on both sides.
All loops are four steps (skip_timesteps = 996); host `out`s are pre-filled with 7.0 so that untouched rows can be seen."""
import ctypes

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.model import ClassifierFreeSampleModel
from tests import clip_queue_edit_util as E                                          # noqa: F401
from tests.clip_queue_session_util import RawSession, _dsgplus_jobs, open_queue
from tests.clip_queue_util import PAIRS, SHARED, SKIP, _zeggs_like, alone, clips_of, diffusion, model, n_out_of, queue_jobs

PENDING, RUNNING, DONE, CANCELLED = L.JOB_PENDING, L.JOB_RUNNING, L.JOB_DONE, L.JOB_CANCELLED


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def jobs_of(cfg, clips, pairs, scales=None):
    """the dicts of `ClipQueue.submit`: the ZEGGS layout takes the features as they are, the DSG+ layout as `_dsgplus_window_y` builds them"""
    return queue_jobs(cfg, clips, pairs, scales) if _zeggs_like(cfg) else _dsgplus_jobs(cfg, clips, pairs, scales)


def head(clip, K):
    """the first K windows of a clip, as a clip"""
    return dict(clip, feats=tuple(clip["feats"][:K]))


def live_job(job, n_given=0):
    """a dict of `submit` as `submit_live` takes it: only the first n_given windows come with it"""
    return dict(job, feats=list(job["feats"][:n_given]))


def live_rows(cfg, capacity, windows_done, keep_last_tail):
    """rows_ready of a live job that is not finished"""
    return max(0, min(n_out_of(cfg, capacity, keep_last_tail), windows_done * cfg.stride - cfg.n_seed))


def filled(cfg, K, keep_last_tail, guard=0):
    return np.full((n_out_of(cfg, K, keep_last_tail) + guard, cfg.njoints), 7.0, np.float32)


def live_state(q, t):
    """(state, windows_done, rows_ready, windows_given, finished) of a live ticket, read from the struct's reserved words as well"""
    j = q.job(t)
    info = L.dsg_queue_job_info()
    q.lib.check(q.lib.cdll.dsg_queue_job(q._q(), int(t), ctypes.byref(info)))
    assert j["live"] and info.reserved[1] & L.JOB_LIVE and info.reserved[0] == j["windows_given"]
    assert bool(info.reserved[1] & L.JOB_FINISHED) == j["finished"] and info.reserved[2] == 0
    return j["state"], j["windows_done"], j["rows_ready"], j["windows_given"], j["finished"]


# ---- 1. live equals alone ---------------------------------------------------------------------------------------------------------------------
def check_live_equals_alone(lib, cfg=C.TINY, prec="bf16", kset="tile", combos=((False, True), (True, False)), B=2):
    """capacity 4, three windows, one appended before each of rounds 0, 1, 2 (the last with last=True), a closed job of K = 2 beside it"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (4, 2)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs)
    n3, n4 = n_out_of(cfg, 3, False), n_out_of(cfg, 4, False)
    for ddim, root_shift in combos:
        out = filled(cfg, 4, False)
        with open_queue(d, mB, B, ddim=ddim, root_shift=root_shift) as q:
            t = q.submit_live(live_job(jobs[0]), 4, out=out)
            tc = q.submit(jobs[1])
            assert live_state(q, t) == (PENDING, 0, 0, 0, False) and q.job(t)["slot"] == -1
            for r in range(3):
                q.append(t, jobs[0]["feats"][r], last=r == 2)
                assert live_state(q, t)[3:] == (r + 1, r == 2)
                assert q.run(1) == 1
                want = (RUNNING, r + 1, live_rows(cfg, 4, r + 1, False), r + 1, False) if r < 2 else (DONE, 3, n3, 3, True)
                assert live_state(q, t) == want, (r, live_state(q, t), want)
                assert q.job(t)["slot"] == 0 and q.job(t)["first_round"] == 0 and q.rows(t).shape == (want[2], cfg.njoints)
            assert q.run(0) == 0 and q.info() == {"rounds_total": 3, "n_pending": 0, "n_running": 0}
            assert "live" not in q.job(tc) and q.job(tc)["state"] == DONE
            got, beside = q.result(t), q.result(tc)
        assert mB.last_kernel_set() == kset and d._draw == 3 * 5
        want = alone(cfg, m1, d, head(clips[0], 3), pairs[0], ddim=ddim, root_shift=root_shift)
        assert m1.last_kernel_set() == kset
        assert got.shape == want.shape == (n3, cfg.njoints) and np.array_equal(got, want), (ddim, root_shift, float(np.max(np.abs(got - want))))
        assert np.array_equal(out[:n3], want) and (out[n3:n4] == 7.0).all() and out.shape[0] == n4
        assert np.array_equal(beside, alone(cfg, m1, d, clips[1], pairs[1], ddim=ddim, root_shift=root_shift))


# ---- 2. sitting out an odd and an even number of rounds --------------------------------------------------------------------------------------
ARRIVE_IDLE = {2: 1, 5: 2}      # session round -> the window of the live job appended before it (window 0 comes with the job); 5: the last


def run_idle_script(cfg, d, lanes, B, jobs, states=None):
    """slot 0: a closed job of K = 6, rounds 0..5; slot 1: a live job whose windows arrive before rounds 0, 2 and 5 -- it sits out round 1
    (an odd number of rounds) and rounds 3 and 4 (an even number).  Returns (the live clip, the neighbour)"""
    with open_queue(d, lanes, B) as q:
        tc = q.submit(jobs[1])
        t = q.submit_live(live_job(jobs[0], 1), 3)
        for r in range(6):
            if r in ARRIVE_IDLE:
                q.append(t, [jobs[0]["feats"][ARRIVE_IDLE[r]]], last=r == 5)
            before = live_state(q, t)
            assert q.run(1) == 1
            if states is not None:
                states.append((r, before, live_state(q, t)))
            assert (q.job(t)["slot"], q.job(tc)["slot"]) == (1, 0) and q.job(tc)["windows_done"] == r + 1
        assert q.run(0) == 0 and q.info() == {"rounds_total": 6, "n_pending": 0, "n_running": 0}
        return q.result(t), q.result(tc)


def check_sitting_out(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """fails on a hand-off that picks the tail buffers by the session's round: after round 1 the live slot's tail would be the other buffer"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (3, 6)), PAIRS[:2]
    states = []
    got, beside = run_idle_script(cfg, d, mB, B, jobs_of(cfg, clips, pairs), states)
    for r, before, after in states:
        if r in (1, 3, 4):                                                           # idle: RUNNING, nothing moved
            assert before == after and after[0] == RUNNING and after[1] == after[3], (r, before, after)
            assert after[2] == live_rows(cfg, 3, after[1], False)
        else:
            assert after[1] == before[1] + 1, (r, before, after)
    assert [s[2][1] for s in states] == [1, 1, 2, 2, 2, 3] and states[-1][2] == (DONE, 3, n_out_of(cfg, 3, False), 3, True)
    want = alone(cfg, m1, d, clips[0], pairs[0])
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    assert np.array_equal(beside, alone(cfg, m1, d, clips[1], pairs[1]))
    return got


# ---- 3. nothing to run ---------------------------------------------------------------------------------------------------------------------------
def check_nothing_to_run(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clip, pair = clips_of(cfg, (2,))[0], PAIRS[0]
    job = jobs_of(cfg, [clip], [pair])[0]
    with open_queue(d, mB, B) as q:
        t = q.submit_live(live_job(job, 1), 2)
        assert q.run(0) == 1 and q.info() == {"rounds_total": 1, "n_pending": 0, "n_running": 1}
        for _ in range(2):                                                           # an idle live job alone runs no round
            assert q.run(0) == 0 and q.run(1) == 0
            assert q.info() == {"rounds_total": 1, "n_pending": 0, "n_running": 1}
            assert live_state(q, t) == (RUNNING, 1, live_rows(cfg, 2, 1, False), 1, False)
        q.append(t, job["feats"][1])
        assert q.run(0) == 1 and q.info()["rounds_total"] == 2
        assert live_state(q, t)[0] == RUNNING                                        # at its capacity, but nobody has said it ends here
        q.finish(t)
        assert live_state(q, t) == (DONE, 2, n_out_of(cfg, 2, False), 2, True) and q.info()["n_running"] == 0
        got = q.result(t)
    assert np.array_equal(got, alone(cfg, m1, d, clip, pair))


# ---- 4. late and early finish, both layouts -------------------------------------------------------------------------------------------------
def check_finish_late(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """without keep_last_tail: `finish` after the last given window has run -- at once, and after the job sat out a round -- is DONE before
    it returns, with every row there already"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (2, 3)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs)
    want = alone(cfg, m1, d, clips[0], pairs[0])
    n2 = n_out_of(cfg, 2, False)
    for idle in (0, 1):
        out = filled(cfg, 3, False)
        with open_queue(d, mB, B) as q:
            t = q.submit_live(live_job(jobs[0], 2), 3, out=out)
            tc = q.submit(jobs[1])
            assert q.run(2 + idle) == 2 + idle
            assert live_state(q, t) == (RUNNING, 2, n2, 2, False)
            with pytest.raises(L.DSGError, match="not done"):
                q.result(t)
            q.finish(t)
            assert live_state(q, t) == (DONE, 2, n2, 2, True)
            q.finish(t)                                                              # (again: a no-op)
            assert q.run(0) == 1 - idle and q.job(tc)["state"] == DONE
            assert np.array_equal(q.result(t), want) and np.array_equal(out[:n2], want) and (out[n2:] == 7.0).all()
            assert np.array_equal(q.result(tc), alone(cfg, m1, d, clips[1], pairs[1]))


def check_finish_keep_last_tail(lib, cfg=C.TINY4, prec="bf16", kset="tile", B=2):
    """the DSG+ layout (keep_last_tail, no root shift): (i) last=True with the final append -- the last window writes its closing S rows;
    (ii) `finish` one round after the last window ran, a neighbour in between -- the closing S rows come from the slot's tail; (iii) as
    (ii) one round later"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (2, 4)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs)
    want = alone(cfg, m1, d, clips[0], pairs[0], root_shift=False)
    S_, n2 = cfg.n_seed, n_out_of(cfg, 2, True)
    assert want.shape == (n2, cfg.njoints)
    for late in (0, 1, 2):
        out = filled(cfg, 3, True)
        with open_queue(d, mB, B, root_shift=False, keep_last_tail=True) as q:
            tc = q.submit(jobs[1])
            t = q.submit_live(live_job(jobs[0], 1), 3, out=out)
            assert q.run(1) == 1
            q.append(t, jobs[0]["feats"][1], last=late == 0)
            assert q.run(1 + late) == 1 + late
            if late:
                assert live_state(q, t) == (RUNNING, 2, n2 - S_, 2, False) and q.job(tc)["windows_done"] == 2 + late
                assert np.array_equal(out[:n2 - S_], want[:n2 - S_]) and (out[n2 - S_:] == 7.0).all()
                q.finish(t)
            assert live_state(q, t) == (DONE, 2, n2, 2, True)
            assert np.array_equal(q.result(t), want), (late, float(np.max(np.abs(q.result(t) - want))))
            assert np.array_equal(out[:n2], want) and (out[n2:] == 7.0).all()
            q.run(0)
            assert np.array_equal(q.result(tc), alone(cfg, m1, d, clips[1], pairs[1], root_shift=False))


# ---- 5. per-window style and scale -------------------------------------------------------------------------------------------------------------
def host_windows(cfg, m, d, clip, pair, styles, scales=None, root_shift=True):
    """the K-call sequence: every window its own style (and y['scale']) through `p_sample_loop`, stitched as sample.py stitches -- the draw
    order of `generate_clip[_dsgplus](windows="host")` after the same `manual_seed`"""
    S_, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
    feats, K = list(clip["feats"]), len(clip["feats"])
    mask = np.ones((1, T), bool)
    d.manual_seed(*pair)
    out = []
    for c in range(K):
        if _zeggs_like(cfg):
            y = S._zeggs_window_y(cfg, feats[c], styles[c], out[-1] if out else None, clip["seed"], False, mask)
        else:
            y = S._dsgplus_window_y(cfg, feats, c, styles[c], clip["seed"] if c == 0 else out[-1][..., -S_:], clip["seed_last"], False, mask)
        if scales is not None:
            y["scale"] = np.array([scales[c]], np.float32)
        s = d.p_sample_loop(m, (1, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=SKIP, init_image=None, progress=False,
                            dump_steps=None, noise=None, const_noise=False)
        if _zeggs_like(cfg):
            S._zeggs_stitch(out, s, S_, root_shift, False)
        else:
            S._dsgplus_stitch(out, s, S_, False)
    if _zeggs_like(cfg):
        return S._zeggs_finish(out, S_, False)[0]
    return S._dsgplus_finish(out, S_, J, K * cfg.stride, 1, False)[0]


def other_style(cfg, style):
    o = np.zeros_like(style)
    o[0, (int(np.argmax(style)) + 2) % cfg.style_dim_in] = 1.0
    return o


def check_window_style_scale(lib, cfg=C.TINY5, prec="bf16", kset="tile", B=2):
    """a guided session: style and scale change at window 1 of a live job of three windows"""
    mB, m1, d = model(lib, cfg, prec, 2 * B, kset), model(lib, cfg, prec, 2, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (3, 2)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs, scales=(2.5, 0.5))
    clip, job, S_ = clips[0], jobs[0], cfg.n_seed
    sty2 = other_style(cfg, clip["style"])
    got = {}
    for change in (False, True):
        with open_queue(d, mB, B, root_shift=False, keep_last_tail=True, guided=True) as q:
            t = q.submit_live(live_job(job, 1), 3)
            tc = q.submit(jobs[1])
            assert q.run(1) == 1
            q.append(t, job["feats"][1], style=sty2 if change else None, scale=1.5 if change else None)
            q.append(t, job["feats"][2], last=True)
            assert q.run(0) == 2
            got[change] = q.result(t).copy()
            beside = q.result(tc)
        assert mB.last_kernel_set() == kset
    guided1 = ClassifierFreeSampleModel(m1)
    audio = list(job["feats"])
    d.manual_seed(*pairs[0])
    const = d.sample_clip(guided1, audio, clip["style"], seed0=clip["seed"], root_shift=False, keep_last_tail=True, skip_timesteps=SKIP,
                          scale=np.array([2.5], np.float32), seed_last=clip["seed_last"])[0]
    assert m1.last_kernel_set() == kset
    assert np.array_equal(got[False], const)
    first = cfg.stride - S_                                                          # the rows window 0 alone decides
    assert np.array_equal(got[True][:first], const[:first]) and not np.array_equal(got[True][first:], const[first:])
    for w in (1, 2):                                                                 # from window 1 on: every window's own rows differ
        rows = slice(w * cfg.stride, (w + 1) * cfg.stride - S_)
        assert not np.array_equal(got[True][rows], const[rows]), w
    want = host_windows(cfg, guided1, d, clip, pairs[0], [clip["style"], sty2, sty2], scales=[2.5, 1.5, 1.5])
    assert m1.last_kernel_set() == kset
    assert np.array_equal(got[True], want), float(np.max(np.abs(got[True] - want)))
    assert np.array_equal(host_windows(cfg, guided1, d, clip, pairs[0], [clip["style"]] * 3, scales=[2.5] * 3), const)      # (the loop itself)
    d.manual_seed(*pairs[1])
    want_c = d.sample_clip(guided1, list(jobs[1]["feats"]), clips[1]["style"], seed0=clips[1]["seed"], root_shift=False, keep_last_tail=True,
                           skip_timesteps=SKIP, scale=np.array([0.5], np.float32), seed_last=clips[1]["seed_last"])[0]
    assert np.array_equal(beside, want_c)


def check_window_style(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """unguided, the ZEGGS layout with the root shift: a style change at window 1; a scale given to an unguided session is not read"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clip, pair = clips_of(cfg, (3,))[0], PAIRS[0]
    job = jobs_of(cfg, [clip], [pair])[0]
    sty2 = other_style(cfg, clip["style"])
    with open_queue(d, mB, B) as q:
        t = q.submit_live(live_job(job, 1), 3)
        q.append(t, [job["feats"][1], job["feats"][2]], style=sty2, scale=3.0, last=True)
        assert q.run(0) == 3
        got = q.result(t)
    const = alone(cfg, m1, d, clip, pair)
    first = cfg.stride - cfg.n_seed
    assert np.array_equal(got[:first], const[:first]) and not np.array_equal(got[first:], const[first:])
    want = host_windows(cfg, m1, d, clip, pair, [clip["style"], sty2, sty2])
    assert m1.last_kernel_set() == kset and np.array_equal(got, want), float(np.max(np.abs(got - want)))
    assert np.array_equal(host_windows(cfg, m1, d, clip, pair, [clip["style"]] * 3), const)


# ---- 6. slots ----------------------------------------------------------------------------------------------------------------------------------
def check_slots(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """one slot: a live job without a window is passed by a later closed job; it takes the slot after its first append; after its finish
    the next pending job takes the slot (HQ_FIRST after a live tail); a cancelled live job leaves its rows and frees the slot"""
    mB, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (2, 1, 2, 3)), PAIRS[:4]
    jobs = jobs_of(cfg, clips, pairs)
    want = [alone(cfg, m1, d, c, p) for c, p in zip(clips, pairs)]
    out3 = filled(cfg, 3, False)
    with open_queue(d, mB, 1) as q:
        t0 = q.submit_live(live_job(jobs[0]), 2)
        t1 = q.submit(jobs[1])
        assert q.run(1) == 1                                                         # ticket 1 passes ticket 0
        assert q.job(t1)["state"] == DONE and q.job(t1)["first_round"] == 0 and live_state(q, t0) == (PENDING, 0, 0, 0, False)
        assert q.run(0) == 0 and q.info() == {"rounds_total": 1, "n_pending": 1, "n_running": 0}
        t2 = q.submit(jobs[2])
        q.append(t0, jobs[0]["feats"][0])
        assert q.run(1) == 1                                                         # the oldest ticket that can be placed
        assert live_state(q, t0)[:2] == (RUNNING, 1) and (q.job(t0)["slot"], q.job(t0)["first_round"]) == (0, 1)
        assert q.job(t2)["state"] == PENDING
        assert q.run(0) == 0                                                         # it keeps the slot while it waits
        q.append(t0, jobs[0]["feats"][1], last=True)
        t3 = q.submit_live(live_job(jobs[3], 1), 3, out=out3)
        assert q.run(0) == 4                                                         # t0's last window, t2's two, t3's first
        assert q.job(t2)["first_round"] == 3 and q.job(t3)["first_round"] == 5 and q.info()["n_running"] == 1
        n1 = live_rows(cfg, 3, 1, False)
        q.cancel(t3)
        assert live_state(q, t3) == (CANCELLED, 1, n1, 1, False) and q.info() == {"rounds_total": 6, "n_pending": 0, "n_running": 0}
        with pytest.raises(ValueError, match=f"ticket {t3} is cancelled"):
            q.append(t3, jobs[3]["feats"][1])
        q.finish(t3)                                                                 # (nothing left to finish)
        assert live_state(q, t3) == (CANCELLED, 1, n1, 1, False)
        t4 = q.submit(jobs[1])                                                       # the slot is free again
        assert q.run(0) == 1 and q.job(t4)["slot"] == 0
        got = [q.result(t) for t in (t0, t1, t2)] + [q.result(t4)]
    assert 0 < n1 < out3.shape[0] and np.array_equal(out3[:n1], want[3][:n1]) and (out3[n1:] == 7.0).all()
    for g, w in zip(got, (want[0], want[1], want[2], want[1])):
        assert np.array_equal(g, w)


# ---- 7. lanes ----------------------------------------------------------------------------------------------------------------------------------
def check_lanes(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """the arrival script of check_sitting_out on 2 lanes x 1 and on 1 lane x 2: the same bits"""
    d = diffusion(lib)
    base = model(lib, cfg, prec, 2, kset)
    clips, pairs = clips_of(cfg, (3, 6)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs)
    per = {}
    for n_lanes, B in ((2, 1), (1, 2)):
        lanes = [base] + [base.clone(B) for _ in range(n_lanes - 1)]
        per[n_lanes] = run_idle_script(cfg, d, lanes, B, jobs)
        assert all(ln.last_kernel_set() == kset for ln in lanes)
    assert np.array_equal(per[2][0], per[1][0]) and np.array_equal(per[2][1], per[1][1])
    m1 = model(lib, cfg, prec, 1, kset)
    assert np.array_equal(per[2][0], alone(cfg, m1, d, clips[0], pairs[0]))


# ---- the raw exports --------------------------------------------------------------------------------------------------------------------------
class RawLive(RawSession):
    """RawSession with the three live exports.  `device`: every pointer a torch device tensor that starts `offset` floats past an
    allocation's start, `guard` rows behind `out`"""

    def _tensor(self, a, device, offset):
        a = np.ascontiguousarray(a)
        if not device:
            return a, a.ctypes.data
        import torch
        flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
        flat[offset:] = torch.from_numpy(a.reshape(-1)).cuda()
        t = flat[offset:]
        assert t.data_ptr() % 16 == (offset * t.element_size()) % 16
        return t, t.data_ptr()

    def submit_live(self, clip, pair, capacity, n_given=0, skip=-1, device=False, offset=0, guard=2, audio=None, expect=0):
        """returns the ticket (or, with `expect`, the refusal's message); the host arrays are kept in self.host[ticket]"""
        cfg = self.cfg
        feats = list(clip["feats"] if audio is None else audio)[:n_given]
        arrays = {"style": np.array(clip["style"], np.float32), "seed0": np.array(clip["seed"], np.float32)}
        if feats:
            arrays["audio"] = np.ascontiguousarray(np.concatenate(feats), np.float32)
        if clip.get("seed_last") is not None:
            arrays["seed_last"] = np.array(clip["seed_last"], np.float32)
        out = np.full((max(n_out_of(cfg, max(capacity, 1), self.keep_last_tail), 1) + guard, cfg.njoints), 7.0, np.float32)
        tensors, ptrs = {}, {}
        for k, v in arrays.items():
            tensors[k], ptrs[k] = self._tensor(v, device, offset)
        out_t, out_p = self._tensor(out, device, offset)
        out = out_t.view(out.shape) if device else out
        job = L.dsg_clip_job()
        job.style, job.seed0, job.audio, job.out = ptrs["style"], ptrs["seed0"], ptrs.get("audio"), out_p
        job.seed_last = ptrs.get("seed_last")
        job.K, job.scale, job.seed, job.stream_id = capacity, 1.0, pair[0], pair[1]
        t = ctypes.c_int64(-1)
        rc = self.lib.cdll.dsg_queue_submit_live(self.q, ctypes.byref(job), n_given, skip, ctypes.byref(t), L.current_stream_ptr() if device else None)
        if expect:
            assert rc == expect and t.value == -1, (rc, t.value)
            return (self.lib.cdll.dsg_last_error() or b"").decode()
        self.lib.check(rc)
        assert t.value == len(self.outs)
        self.keep.append([tensors])
        self.outs.append(out)
        self.host.append(arrays)
        return int(t.value)

    def append(self, t, windows, styles=None, flags=None, device=False, offset=0, expect=0, null_audio=()):
        """windows: per-window features; styles: None or one entry (array or None) per window; flags: one int per window.  Returns the
        host arrays it passed (or, with `expect`, the refusal's message)"""
        n = len(windows)
        arr = (L.dsg_queue_window * max(n, 1))()
        host, keep = [], []
        for i, w in enumerate(windows):
            a = np.array(w, np.float32).reshape(self.cfg.audio_frames, self.cfg.audio_src_dim)
            ten, p = self._tensor(a, device, offset)
            host.append(a)
            keep.append(ten)
            arr[i].audio = None if i in null_audio else p
            if styles is not None and styles[i] is not None:
                s = np.array(styles[i], np.float32)
                ten, p = self._tensor(s, device, offset)
                host.append(s)
                keep.append(ten)
                arr[i].style = p
            arr[i].flags = 0 if flags is None else flags[i]
        rc = self.lib.cdll.dsg_queue_append(self.q, t, arr, n, L.current_stream_ptr() if device else None)
        if expect:
            assert rc == expect, rc
            return (self.lib.cdll.dsg_last_error() or b"").decode()
        self.lib.check(rc)
        self.keep[t].append(keep)
        return host

    def finish(self, t, expect=0):
        rc = self.lib.cdll.dsg_queue_finish(self.q, t)
        if expect:
            assert rc == expect, rc
            return (self.lib.cdll.dsg_last_error() or b"").decode()
        self.lib.check(rc)

    def job(self, t):
        info = L.dsg_queue_job_info()
        self.lib.check(self.lib.cdll.dsg_queue_job(self.q, t, ctypes.byref(info)))
        return info.state, info.windows_done, info.rows_ready, info.reserved[0], info.reserved[1]


# ---- 8. ownership ---------------------------------------------------------------------------------------------------------------------------
def check_inputs_free(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """every host tensor of submit_live and of every append -- audio, style, seed0 -- overwritten with NaN right after the call"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    mB.set_schedule(d)
    clips, pairs = clips_of(cfg, (3, 2)), PAIRS[:2]
    s = RawLive(lib, [mB.handle], cfg, B)
    assert s.rc == 0, s.msg
    try:
        t = s.submit_live(clips[0], pairs[0], 3, n_given=1)
        for a in s.host[t].values():
            a.fill(np.nan)
        assert s.submit(clips[1], pairs[1]) == 1
        assert s.run(1) == 1
        for c in (1, 2):
            # (window 1 brings the job's own style again, as a tensor of its own)
            host = s.append(t, [clips[0]["feats"][c]], styles=[clips[0]["style"]] if c == 1 else None, flags=[L.WIN_LAST if c == 2 else 0])
            for a in host:
                a.fill(np.nan)
            assert s.run(1) == 1
        assert s.job(t) == (DONE, 3, n_out_of(cfg, 3, False), 3, L.JOB_LIVE | L.JOB_FINISHED)
        got, beside = s.out(t), s.out(1)
    finally:
        s.close()
    assert np.array_equal(got[:-2], alone(cfg, m1, d, clips[0], pairs[0])) and (got[-2:] == 7.0).all()
    assert np.array_equal(beside[:-2], alone(cfg, m1, d, clips[1], pairs[1]))


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """each with its message and ticket; a refused append takes nothing: the job still completes and equals alone"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    mB.set_schedule(d)
    clips, pairs = clips_of(cfg, (3, 1, 1)), PAIRS[:3]
    w = clips[0]["feats"]
    INV = L.E_INVALID
    s = RawLive(lib, [mB.handle], cfg, B)
    assert s.rc == 0, s.msg
    try:
        assert "job 0 has K < 1" in s.submit_live(clips[0], pairs[0], 0, expect=INV)
        assert "job 0 brings 3 windows for a capacity of 2" in s.submit_live(clips[0], pairs[0], 2, n_given=3, expect=INV)
        assert "n_given < 0" in s.submit_live(clips[0], pairs[0], 2, n_given=-1, expect=INV)
        assert "job 0 has skip_timesteps 1000" in s.submit_live(clips[0], pairs[0], 2, skip=1000, expect=INV)
        t = s.submit_live(clips[0], pairs[0], 3, n_given=1)                         # a refused submit took no ticket
        closed = s.submit(clips[1], pairs[1])
        gone = s.submit_live(clips[2], pairs[2], 2, n_given=1)
        assert (t, closed, gone) == (0, 1, 2)
        assert lib.cdll.dsg_queue_cancel(s.q, gone) == 0
        assert f"ticket {t}: 1 + 3 windows exceed the capacity of 3" in s.append(t, [w[1], w[2], w[2]], expect=INV)
        assert f"ticket {closed} is not a live job" in s.append(closed, [w[1]], expect=INV)
        assert f"ticket {gone} is cancelled" in s.append(gone, [w[1]], expect=INV)
        assert "no such ticket: 3" in s.append(3, [w[1]], expect=INV) and "no such ticket: -1" in s.append(-1, [w[1]], expect=INV)
        assert f"ticket {t}: n < 1" in s.append(t, [], expect=INV)
        assert f"ticket {t}: window 1 has a null audio" in s.append(t, [w[1], w[2]], null_audio=(1,), expect=INV)
        assert f"ticket {t}: DSG_WIN_LAST on window 0 of 2" in s.append(t, [w[1], w[2]], flags=[L.WIN_LAST, 0], expect=INV)
        assert lib.cdll.dsg_queue_append(s.q, t, None, 1, None) == INV
        assert "no such ticket: 3" in s.finish(3, expect=INV) and f"ticket {closed} is not a live job" in s.finish(closed, expect=INV)
        assert s.job(t) == (PENDING, 0, 0, 1, L.JOB_LIVE)                            # the refusals took nothing
        assert s.run(1) == 1
        s.append(t, [w[1], w[2]], flags=[0, L.WIN_LAST])
        assert f"ticket {t} is finished" in s.append(t, [w[2]], expect=INV)
        assert s.run(0) == 2
        assert f"ticket {t} is done" in s.append(t, [w[2]], expect=INV)
        s.finish(t)                                                                  # finished already: a no-op
        assert s.job(t) == (DONE, 3, n_out_of(cfg, 3, False), 3, L.JOB_LIVE | L.JOB_FINISHED)
        # a live job finished without a window is cancelled
        empty = s.submit_live(clips[2], pairs[2], 2)
        s.finish(empty)
        assert s.job(empty) == (CANCELLED, 0, 0, 0, L.JOB_LIVE | L.JOB_FINISHED) and s.run(0) == 0
        got = s.out(t)
    finally:
        s.close()
    assert np.array_equal(got[:-2], alone(cfg, m1, d, clips[0], pairs[0])) and (got[-2:] == 7.0).all()
    # the Python layer: edits are refused before the library is asked
    with open_queue(d, mB, B) as q:
        job = jobs_of(cfg, clips[:1], pairs[:1])[0]
        with pytest.raises(ValueError, match="takes no edits"):
            q.submit_live(dict(live_job(job), init_motion=np.zeros((n_out_of(cfg, 3, False), cfg.njoints), np.float32)), 3)
        with pytest.raises(ValueError, match="has K < 1"):
            q.submit_live(live_job(job), 0)


# ---- 10. ABI -----------------------------------------------------------------------------------------------------------------------------------
def check_abi(lib):
    assert lib.cdll.dsg_version() == 330
    assert ctypes.sizeof(L.dsg_queue_window) == 32
    assert [f[0] for f in L.dsg_queue_window._fields_] == ["audio", "style", "scale", "flags", "reserved"]
    assert ctypes.sizeof(L.dsg_queue_job_info) == 32 and ctypes.sizeof(L.dsg_clip_job) == 80 and ctypes.sizeof(L.dsg_clip_edit) == 32
    for name in ("dsg_queue_submit_live", "dsg_queue_append", "dsg_queue_finish"):
        assert name in L.SYMBOLS and hasattr(lib.cdll, name)
    assert (L.WIN_SCALE, L.WIN_LAST, L.JOB_LIVE, L.JOB_FINISHED) == (1, 2, 1, 2)
    assert lib.cdll.dsg_queue_finish(None, 0) == L.E_INVALID and lib.cdll.dsg_queue_append(None, 0, None, 1, None) == L.E_INVALID


# ---- the drivers of sample.py ------------------------------------------------------------------------------------------------------------------
def check_drivers(lib, prec="bf16", kset="tile"):
    """`open_clip_queue` and `open_clip_queue_dsgplus`: submit_live / append / finish, the DSG+ crop given at finish"""
    # the attention3 layout of the DSG+ tree puts the tail of the window before in front of a window's features: across appends too (host only)
    cfg, rs = C.TINY3B, np.random.RandomState(3)
    feats = [rs.randn(1, cfg.stride, cfg.audio_src_dim).astype(np.float32) for _ in range(4)]
    seed = np.zeros((1, cfg.njoints, 1, cfg.n_seed), np.float32)
    drv = S._ClipQueueSession.__new__(S._ClipQueueSession)
    drv.cfg, drv.dsgplus, drv._live = cfg, True, {0: [seed, None, None]}
    fed = drv._window_audio(0, feats[:1]) + drv._window_audio(0, feats[1:3]) + drv._window_audio(0, feats[3])
    whole = [S._dsgplus_window_y(cfg, feats, w, None, seed, None, False, None)["audio"] for w in range(4)]
    assert len(fed) == 4 and all(np.array_equal(a, b) for a, b in zip(fed, whole)) and fed[1].shape[1] == cfg.n_poses
    for cfg in (C.TINY, C.TINY5):
        mB, m1, d = model(lib, cfg, prec, 2, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
        clip, sid = clips_of(cfg, (3,))[0], PAIRS[0][1]
        base = {"style": clip["style"][0] if _zeggs_like(cfg) else clip["style"], "seed_pose": clip["seed"], "clip_id": sid}
        if _zeggs_like(cfg):
            with S.open_clip_queue(mB, d, seed=SHARED, skip_timesteps=SKIP, kernel_set=kset) as q:
                t = q.submit_live(dict(base, feats=[clip["feats"][0]]), 4)
                assert q.run(0) == 1
                q.append(t, list(clip["feats"][1:]), last=True)
                assert q.run(0) == 2
                got = q.result(t)
            want = alone(cfg, m1, d, clip, (SHARED, sid))
        else:
            real = 3 * cfg.stride - 5
            with S.open_clip_queue_dsgplus(mB, d, seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=kset, B=2) as q:
                t = q.submit_live(dict(base, seed_last=clip["seed_last"], feats=[]), 4)
                for c in range(3):
                    q.append(t, clip["feats"][c])
                    assert q.run(0) == 1
                assert q.rows(t).shape == (3 * cfg.stride - cfg.n_seed, cfg.njoints)
                q.finish(t, real_n_frames=real)
                got = q.result(t)
            want = alone(cfg, m1, d, clip, (SHARED, sid), root_shift=False)[:real]
        assert got.shape == want.shape and np.array_equal(got, want), cfg.name


# ---- 11. GPU only ------------------------------------------------------------------------------------------------------------------------------
def check_zeggs_rows(lib):
    """ZEGGS widths, bf16, the ROWS set, B = 3: a live job sits out round 1 beside two closed jobs"""
    cfg, B = C.ZEGGS, 3
    mB, m1, d = model(lib, cfg, "bf16", B, "rows"), model(lib, cfg, "bf16", 1, "rows"), diffusion(lib)
    clips, pairs = clips_of(cfg, (2, 3, 1)), PAIRS[:3]
    jobs = jobs_of(cfg, clips, pairs)
    with open_queue(d, mB, B) as q:
        t = q.submit_live(live_job(jobs[0], 1), 2)
        tc = [q.submit(jobs[1]), q.submit(jobs[2])]
        assert q.run(2) == 2 and live_state(q, t)[:2] == (RUNNING, 1)
        q.append(t, jobs[0]["feats"][1], last=True)
        assert q.run(0) == 1 and q.info()["rounds_total"] == 3
        got = [q.result(x) for x in [t] + tc]
    assert mB.last_kernel_set() == "rows"
    for i in range(3):
        want = alone(cfg, m1, d, clips[i], pairs[i])
        assert m1.last_kernel_set() == "rows"
        assert np.array_equal(got[i], want), (i, float(np.max(np.abs(got[i] - want))))


def check_device_pointers(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """every pointer of submit_live and append a device tensor that starts one float past a 16-byte boundary, two guard rows behind `out`:
    the run equals the host-pointer run"""
    m, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    m.set_schedule(d)
    clips, pairs = clips_of(cfg, (3, 2)), PAIRS[:2]
    sty2 = other_style(cfg, clips[0]["style"])
    res = {}
    for device in (False, True):
        off = 1 if device else 0
        s = RawLive(lib, [m.handle], cfg, B)
        assert s.rc == 0, s.msg
        try:
            t = s.submit_live(clips[0], pairs[0], 3, n_given=1, device=device, offset=off)
            tc = s.submit(clips[1], pairs[1], device=device, offset=off)
            assert s.run(2, device) == 2                                             # the live job sits out round 1
            s.append(t, clips[0]["feats"][1:], styles=[None, sty2], flags=[0, L.WIN_LAST], device=device, offset=off)
            assert s.run(0, device) == 2
            res[device] = [s.out(t), s.out(tc)]
        finally:
            s.close()
    for i in range(2):
        assert np.array_equal(res[True][i], res[False][i]) and (res[True][i][-2:] == 7.0).all(), i
    want = host_windows(cfg, m1, d, clips[0], pairs[0], [clips[0]["style"], clips[0]["style"], sty2])
    assert np.array_equal(res[False][0][:-2], want)
    assert np.array_equal(res[False][1][:-2], alone(cfg, m1, d, clips[1], pairs[1]))
