"""Shared by tests/test_emu_clip_queue_prio.py (CPU, the SIMT emulator) and tests/test_gpu_clip_queue_prio.py (MI355X): the checks of job
priorities, park and resume in a queue session (dsg_queue_set_priority / _park / _resume / dsg_queue_place_prio; `ClipQueue.submit(...,
priority=)`, `set_priority`, `park`, `resume` and the two drivers of sample.py), written once over a `DSGLibrary`.  Every comparison of
motion is `np.array_equal`: a clip out of the session -- however often it left its slot, whichever slot and lane it came back to -- against
the same clip sampled alone on a batch-1 handle through the existing clip drivers (`windows="library"`) with the same kernel set named on
both sides.  All loops are four steps (skip_timesteps = 996) unless a clip brings its own skip; host `out`s are pre-filled with 7.0 so that
untouched rows can be seen."""
import ctypes

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.model import ClassifierFreeSampleModel
from diffusestylegesture_amd.synth import synth_window_inputs
from tests import clip_queue_edit_util as E
from tests.clip_queue_edit_util import BOTH, INIT, NONE, edits_of
from tests.clip_queue_live_util import filled, jobs_of, live_job, live_rows
from tests.clip_queue_session_util import RawSession, open_queue, rows_ready_of, run_arrivals
from tests.clip_queue_util import PAIRS, SHARED, SKIP, _after, _zeggs_like, alone, clips_of, diffusion, model, n_out_of

PENDING, RUNNING, DONE, CANCELLED, PARKED = L.JOB_PENDING, L.JOB_RUNNING, L.JOB_DONE, L.JOB_CANCELLED, L.JOB_PARKED


def raw_info(q, t):
    info = L.dsg_queue_job_info()
    q.lib.check(q.lib.cdll.dsg_queue_job(q._q(), int(t), ctypes.byref(info)))
    return info


def st(q, t):
    """(state, slot, windows_done, parks, held) of a ticket; the dict of `job` agrees with the struct's words"""
    j, info = q.job(t), raw_info(q, t)
    assert (info.state, info.slot, info.windows_done, info.reserved[2]) == (j["state"], j["slot"], j["windows_done"], j["parks"])
    assert bool(info.reserved[1] & L.JOB_HELD) == j["held"]
    return j["state"], j["slot"], j["windows_done"], j["parks"], j["held"]


def layout(cfg):
    """(root_shift, keep_last_tail) of the layout the config's clips are stitched in"""
    return (True, False) if _zeggs_like(cfg) else (False, True)


# ---- 1. order -----------------------------------------------------------------------------------------------------------------------------------
def check_order(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """one slot; A (K 3, prio 0), B (K 1, prio 0), C (K 1, prio 5) submitted before the first round: C runs first, then A, then B"""
    mB, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (3, 1, 1)), PAIRS[:3]
    jobs = jobs_of(cfg, clips, pairs)
    with open_queue(d, mB, 1) as q:
        t = [q.submit(jobs[0]), q.submit(jobs[1], priority=0), q.submit(dict(jobs[2], priority=5))]
        assert [q.job(x)["priority"] for x in t] == [0, 0, 5]
        assert q.run(0) == 5
        assert [q.job(x)["first_round"] for x in t] == [1, 4, 0] and [q.job(x)["parks"] for x in t] == [0, 0, 0]
        got = [q.result(x) for x in t]
    assert L.queue_place_prio((3, 1, 1), 1, None, (0, 0, 5), lib) == ([1, 4, 0], [3, 4, 0], [0, 0, 0], 5)
    assert mB.last_kernel_set() == kset
    for i in range(3):
        assert np.array_equal(got[i], alone(cfg, m1, d, clips[i], pairs[i])), i


# ---- 2. pre-emption -----------------------------------------------------------------------------------------------------------------------------
def check_preempt(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """one slot; A (K 4) runs one round, H (K 2, prio 1) arrives: A is parked with its rows so far, H runs, A comes back and finishes"""
    mB, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (4, 2)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs)
    want = [alone(cfg, m1, d, c, p) for c, p in zip(clips, pairs)]
    out = filled(cfg, 4, False)
    n1 = rows_ready_of(cfg, 4, 1, False)
    with open_queue(d, mB, 1) as q:
        a = q.submit(jobs[0], out=out)
        assert q.run(1) == 1 and st(q, a) == (RUNNING, 0, 1, 0, False) and q.job(a)["rows_ready"] == n1
        h = q.submit(jobs[1], priority=1)
        assert q.run(1) == 1
        assert st(q, a) == (PARKED, -1, 1, 1, False) and q.job(a)["rows_ready"] == n1 and q.job(a)["first_round"] == 0
        assert 0 < n1 < out.shape[0] and np.array_equal(out[:n1], want[0][:n1]) and (out[n1:] == 7.0).all()
        assert st(q, h) == (RUNNING, 0, 1, 0, False) and q.info() == {"rounds_total": 2, "n_pending": 1, "n_running": 1}
        assert q.run(1) == 1 and q.job(h)["state"] == DONE and st(q, a) == (PARKED, -1, 1, 1, False)
        assert q.run(1) == 1 and st(q, a) == (RUNNING, 0, 2, 1, False)
        assert q.run(0) == 2 and q.run(0) == 0
        rounds = q.info()["rounds_total"]
        first, parks = [q.job(x)["first_round"] for x in (a, h)], [q.job(x)["parks"] for x in (a, h)]
        got = [q.result(a), q.result(h)]
    assert (first, [5, 2], parks, rounds) == L.queue_place_prio((4, 2), 1, (0, 1), (0, 1), lib)
    assert mB.last_kernel_set() == kset
    assert np.array_equal(got[0], want[0]) and np.array_equal(out, want[0]) and np.array_equal(got[1], want[1])


# ---- 3. the parity of the tail buffer; 7. lanes --------------------------------------------------------------------------------------------------
def run_parity_script(lib, cfg, d, lanes, jobs, after):
    """two slots.  Slot 0: A (K 4, prio 0); slot 1: a neighbour N (K after + 1, prio 1).  After `after` rounds H (K 3, prio 2) arrives and
    takes A's slot: A is parked on window `after` and reads its tail from clip_tail[(after - 1) & 1].  N ends in that round, so A comes
    back in the OTHER slot (on two lanes: the other lane) while H still holds its old one.  Returns the clips of A, N, H"""
    B = 2 // len(lanes)
    root_shift, keep_last_tail = layout(cfg)
    with open_queue(d, lanes, B, root_shift=root_shift, keep_last_tail=keep_last_tail) as q:
        a, n = q.submit(jobs[0]), q.submit(jobs[1])
        assert q.run(after) == after and st(q, a) == (RUNNING, 0, after, 0, False) and st(q, n) == (RUNNING, 1, after, 0, False)
        q.set_priority(n, 1)                                                         # (in its slot already: A is the one to go)
        h = q.submit(jobs[2], priority=2)
        assert q.run(1) == 1
        assert st(q, a) == (PARKED, -1, after, 1, False) and st(q, h) == (RUNNING, 0, 1, 0, False) and q.job(n)["state"] == DONE
        assert q.job(a)["rows_ready"] == rows_ready_of(cfg, 4, after, keep_last_tail)
        assert q.run(1) == 1 and st(q, a) == (RUNNING, 1, after + 1, 1, False) and st(q, h) == (RUNNING, 0, 2, 0, False)
        assert q.run(0) == 5 - after - 2 and q.info() == {"rounds_total": 5, "n_pending": 0, "n_running": 0}
        assert [q.job(x)["first_round"] for x in (a, n, h)] == [0, 0, after]
        got = [q.result(x) for x in (a, n, h)]
    assert L.queue_place_prio((4, after + 1, 3), 2, (0, 0, after), (0, 1, 2), lib) == ([0, 0, after], [4, after, after + 2], [1, 0, 0], 5)
    return got


def beatpp_clips(Ks, first_id=20):
    """as clip_queue_util.clip_of at the BEAT++ widths, with the stride-long windows of the DSG+ config of the same widths"""
    cfg, clips = C.BEATPP, []
    for i, K in enumerate(Ks):
        cid = first_id + i
        y0 = synth_window_inputs(cfg, 1, window=0, clips=[cid], seed_pose_scale=0.3)
        style = np.zeros((1, cfg.style_dim_in), np.float32)
        style[0, cid % cfg.style_dim_in] = 1.0
        clips.append({"feats": tuple(synth_window_inputs(C.BEAT, 1, window=w, clips=[cid])["audio"] for w in range(K)), "style": style,
                      "seed": y0["seed"], "seed_last": y0["seed_last"]})
    return clips


def check_tail_parity(lib, cfg=C.TINY, prec="bf16", kset="tile", afters=(1, 2), lane_shapes=(1,)):
    """A is parked after one window and, in a second run, after two: an odd and an even tail buffer.  lane_shapes: the number of lanes the
    two slots are spread over -- 2: parked on lane 0, resumed on lane 1"""
    d = diffusion(lib)
    m1 = model(lib, cfg, prec, 1, kset)
    base = model(lib, cfg, prec, 2, kset)
    root_shift, _ = layout(cfg)
    for after in afters:
        Ks = (4, after + 1, 3)
        clips, pairs = (beatpp_clips(Ks) if cfg is C.BEATPP else clips_of(cfg, Ks)), PAIRS[:3]
        jobs = jobs_of(cfg, clips, pairs)
        want = [alone(cfg, m1, d, c, p, root_shift=root_shift) for c, p in zip(clips, pairs)]
        assert m1.last_kernel_set() == kset
        for n_lanes in lane_shapes:
            lanes = [base] + [base.clone(2 // n_lanes) for _ in range(n_lanes - 1)]      # (the clone shares the weights)
            got = run_parity_script(lib, cfg, d, lanes, jobs, after)
            assert all(ln.last_kernel_set() == kset for ln in lanes)
            for i in range(3):
                assert np.array_equal(got[i], want[i]), (cfg.name, after, n_lanes, i, float(np.max(np.abs(got[i] - want[i]))))


def check_lanes(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    check_tail_parity(lib, cfg, prec, kset, afters=(1,), lane_shapes=(2,))      # (one lane x 2: check_tail_parity itself)


# ---- 4. equal priorities change nothing ------------------------------------------------------------------------------------------------------
def check_equal_priorities(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3, 1, 1, 2), arrive=(0, 0, 0, 1, 1, 2), B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    slot, first, n_rounds = L.queue_place(Ks, B, arrive, lib)
    per = {}
    for prio in (0, 3):
        jobs = [dict(j, priority=prio) for j in jobs_of(cfg, clips, pairs)]
        seen = []
        with open_queue(d, mB, B) as q:
            def table(rounds_done, tickets, q=q):
                seen.extend(raw_info(q, t).state for t in tickets)
            tickets = run_arrivals(q, jobs, arrive, each_round=table)
            assert q.info() == {"rounds_total": n_rounds, "n_pending": 0, "n_running": 0}
            assert [(q.job(t)["slot"], q.job(t)["first_round"]) for t in tickets] == list(zip(slot, first))
            assert all(q.job(t)["priority"] == prio and q.job(t)["parks"] == 0 and not q.job(t)["held"] for t in tickets)
            assert all(raw_info(q, t).reserved[2] == 0 and raw_info(q, t).reserved[1] == 0 for t in tickets)
            assert seen and PARKED not in seen
            per[prio] = [q.result(t) for t in tickets]
    assert L.queue_place_prio(Ks, B, arrive, None, lib)[0] == first and L.queue_place_prio(Ks, B, arrive, [3] * len(Ks), lib)[0] == first
    for i in range(len(Ks)):
        assert np.array_equal(per[0][i], per[3][i]), i
    for i in (2, 5):
        assert np.array_equal(per[0][i], alone(cfg, m1, d, clips[i], pairs[i])), i


# ---- 5. explicit park / resume -----------------------------------------------------------------------------------------------------------------
def check_park_resume(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """one slot.  A running job is parked by the caller: it leaves at the next round and the pending ticket takes the slot; held jobs alone
    run no round; resumed, it finishes.  A held PENDING job is passed by the ticket behind it until it is resumed"""
    mB, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (3, 1, 1, 1)), PAIRS[:4]
    jobs = jobs_of(cfg, clips, pairs)
    with open_queue(d, mB, 1) as q:
        a, p = q.submit(jobs[0]), q.submit(jobs[1])
        assert q.run(1) == 1
        q.park(a)
        assert st(q, a) == (RUNNING, 0, 1, 0, True)                                  # held: it leaves when the next round starts
        q.park(a)                                                                    # (again: a no-op)
        assert q.run(1) == 1
        assert st(q, a) == (PARKED, -1, 1, 1, True) and q.job(p)["state"] == DONE and q.job(p)["slot"] == 0
        for _ in range(2):                                                           # held jobs alone run no round
            assert q.run(0) == 0 and q.run(1) == 0
            assert q.info() == {"rounds_total": 2, "n_pending": 1, "n_running": 0} and st(q, a) == (PARKED, -1, 1, 1, True)
        q.park(a)                                                                    # (parked and held already)
        q.resume(a)
        assert st(q, a) == (PARKED, -1, 1, 1, False)
        q.resume(a)                                                                  # (not held: a no-op)
        assert q.run(0) == 2 and st(q, a) == (DONE, 0, 3, 1, False)
        # a held pending job
        x, y = q.submit(jobs[2]), q.submit(jobs[3])
        q.park(x)
        assert st(q, x) == (PENDING, -1, 0, 0, True)
        assert q.run(0) == 1 and q.job(y)["state"] == DONE and st(q, x) == (PENDING, -1, 0, 0, True)
        assert q.run(0) == 0 and q.info() == {"rounds_total": 5, "n_pending": 1, "n_running": 0}
        q.resume(x)
        assert q.run(0) == 1 and st(q, x) == (DONE, 0, 1, 0, False) and q.job(x)["first_round"] == 5
        got = [q.result(t) for t in (a, p, x, y)]
    assert mB.last_kernel_set() == kset
    for i in range(4):
        assert np.array_equal(got[i], alone(cfg, m1, d, clips[i], pairs[i])), i


# ---- 6. live jobs --------------------------------------------------------------------------------------------------------------------------------
def check_live_victim(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """an idle live job (ticket 0) is the victim before a busy job of the same priority with a higher ticket; after `append` it returns
    once a slot is free and equals its windows alone"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (3, 4, 1)), PAIRS[:3]
    jobs = jobs_of(cfg, clips, pairs)
    out = filled(cfg, 3, False)
    with open_queue(d, mB, B) as q:
        lv = q.submit_live(live_job(jobs[0], 1), 3, out=out)
        busy = q.submit(jobs[1])
        assert q.run(1) == 1 and st(q, lv) == (RUNNING, 0, 1, 0, False)
        h = q.submit(jobs[2], priority=1)
        assert q.run(1) == 1                                                         # the live job has no window: it goes, the busy one stays
        assert st(q, lv) == (PARKED, -1, 1, 1, False) and st(q, busy) == (RUNNING, 1, 2, 0, False) and st(q, h) == (DONE, 0, 1, 0, False)
        assert q.job(lv)["rows_ready"] == live_rows(cfg, 3, 1, False)
        assert q.run(1) == 1 and st(q, lv) == (PARKED, -1, 1, 1, False)              # parked without a window: it cannot be placed
        q.append(lv, jobs[0]["feats"][1])
        assert q.run(1) == 1 and st(q, lv) == (RUNNING, 0, 2, 1, False)
        q.append(lv, jobs[0]["feats"][2], last=True)
        assert q.run(0) == 1 and q.job(lv)["state"] == DONE and q.job(busy)["state"] == DONE
        got = [q.result(x) for x in (lv, busy, h)]
    assert mB.last_kernel_set() == kset
    for i in range(3):
        assert np.array_equal(got[i], alone(cfg, m1, d, clips[i], pairs[i])), i
    assert np.array_equal(out, got[0])


def check_live_finish_parked(lib, cfg=C.TINY4, prec="bf16", kset="tile", B=2):
    """`finish` on a parked live job whose windows have all run: DONE at once.  The DSG+ layout (keep_last_tail): the closing S rows come
    from the parked block; the ZEGGS layout: every row is there already"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (2, 4)), PAIRS[:2]
    jobs = jobs_of(cfg, clips, pairs)
    root_shift, klt = layout(cfg)
    want = alone(cfg, m1, d, clips[0], pairs[0], root_shift=root_shift)
    n2, S_ = n_out_of(cfg, 2, klt), cfg.n_seed
    out = filled(cfg, 3, klt)
    with open_queue(d, mB, B, root_shift=root_shift, keep_last_tail=klt) as q:
        lv = q.submit_live(live_job(jobs[0], 2), 3, out=out)
        busy = q.submit(jobs[1])
        assert q.run(2) == 2
        q.park(lv)
        assert q.run(1) == 1 and st(q, lv) == (PARKED, -1, 2, 1, True)
        ready = n2 - S_ if klt else n2
        assert q.job(lv)["rows_ready"] == ready and (out[ready:] == 7.0).all()
        q.finish(lv)
        assert st(q, lv) == (DONE, -1, 2, 1, False) and q.job(lv)["rows_ready"] == n2 and q.job(lv)["finished"]
        assert q.info() == {"rounds_total": 3, "n_pending": 0, "n_running": 1}
        assert np.array_equal(q.result(lv), want), float(np.max(np.abs(q.result(lv) - want)))
        assert np.array_equal(out[:n2], want) and (out[n2:] == 7.0).all()
        assert q.run(0) == 1
        assert np.array_equal(q.result(busy), alone(cfg, m1, d, clips[1], pairs[1], root_shift=root_shift))


# ---- 8. everything a job can carry -------------------------------------------------------------------------------------------------------------
def check_everything(lib, cfg=C.TINY, prec="bf16", kset="tile", B=2):
    """a guided session.  A: scale 2.5, its own skip_timesteps, an inpainting constraint and an init motion -- parked after window 1 and
    resumed; N beside it: scale 0.0 and an init motion; H: the job that takes A's slot.  The ZEGGS layout runs with the root shift, the
    DSG++ layout (variant 5) without"""
    mB, m1, d = model(lib, cfg, prec, 2 * B, kset), model(lib, cfg, prec, 2, kset), diffusion(lib)
    root_shift, klt = layout(cfg)
    Ks, kinds, scales, skips, prios = (3, 3, 1), (BOTH, INIT, NONE), (2.5, 0.0, 1.0), (998, SKIP, SKIP), (0, 1, 2)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:3]
    edits = edits_of(cfg, Ks, klt, kinds)
    jobs = [dict(j, **e, **({} if s == SKIP else {"skip_timesteps": s})) for j, e, s in zip(jobs_of(cfg, clips, pairs, scales), edits, skips)]
    with open_queue(d, mB, B, root_shift=root_shift, keep_last_tail=klt, guided=True) as q:
        a, n = q.submit(jobs[0]), q.submit(jobs[1])
        assert q.run(1) == 1
        q.set_priority(n, prios[1])
        h = q.submit(jobs[2], priority=prios[2])
        assert q.run(1) == 1 and st(q, a) == (PARKED, -1, 1, 1, False) and st(q, h) == (DONE, 0, 1, 0, False)
        assert q.run(1) == 1 and st(q, a) == (RUNNING, 0, 2, 1, False)
        assert q.run(0) == 1 and q.info() == {"rounds_total": 4, "n_pending": 0, "n_running": 0}
        got = [q.result(x) for x in (a, n, h)]
    assert mB.last_kernel_set() == kset
    guided1 = ClassifierFreeSampleModel(m1)
    for i in range(3):
        d.manual_seed(*pairs[i])
        want = d.sample_clip(guided1, list(jobs[i]["feats"]), clips[i]["style"], seed0=clips[i]["seed"], root_shift=root_shift, keep_last_tail=klt,
                             skip_timesteps=skips[i], scale=np.array([scales[i]], np.float32), seed_last=clips[i]["seed_last"],
                             **E._b1(edits[i]))[0]
        assert m1.last_kernel_set() == kset
        assert np.array_equal(got[i], want), (cfg.name, i, float(np.max(np.abs(got[i] - want))))


# ---- 9. housekeeping -----------------------------------------------------------------------------------------------------------------------------
def check_cancel_parked(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """`cancel` on a parked job: CANCELLED, its rows stay, nobody else is affected and a job submitted afterwards (which takes the staging
    the cancelled one gave back) equals alone"""
    mB, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, (3, 2, 2)), PAIRS[:3]
    jobs = jobs_of(cfg, clips, pairs)
    out = filled(cfg, 3, False)
    n1 = rows_ready_of(cfg, 3, 1, False)
    with open_queue(d, mB, 1) as q:
        a = q.submit(jobs[0], out=out)
        assert q.run(1) == 1
        h = q.submit(jobs[1], priority=1)
        assert q.run(1) == 1 and st(q, a) == (PARKED, -1, 1, 1, False) and q.info()["n_pending"] == 1
        q.cancel(a)
        assert st(q, a) == (CANCELLED, -1, 1, 1, False) and q.info() == {"rounds_total": 2, "n_pending": 0, "n_running": 1}
        q.cancel(a)
        for call in (q.park, q.resume):                                              # a cancelled job: no-ops
            call(a)
        q.set_priority(a, 9)
        assert st(q, a) == (CANCELLED, -1, 1, 1, False) and q.job(a)["priority"] == 0
        n = q.submit(jobs[2])
        assert q.run(0) == 3 and q.job(n)["first_round"] == 3
        q.set_priority(h, 4)                                                         # a done job: a no-op
        q.park(h)
        assert st(q, h) == (DONE, 0, 2, 0, False) and q.job(h)["priority"] == 1
        got = [q.result(h), q.result(n)]
        with pytest.raises(L.DSGError, match="not done"):
            q.result(a)
    want = alone(cfg, m1, d, clips[0], pairs[0])
    assert np.array_equal(out[:n1], want[:n1]) and (out[n1:] == 7.0).all()
    for g, i in zip(got, (1, 2)):
        assert np.array_equal(g, alone(cfg, m1, d, clips[i], pairs[i])), i


def check_close_parked(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """`close` with a parked job, a held running one and a held pending one: the lanes sample afterwards what a fresh handle samples"""
    d = diffusion(lib)
    fresh = _after(lib, cfg, model(lib, cfg, prec, 2, kset), d)
    m = model(lib, cfg, prec, 2, kset)
    clips, pairs = clips_of(cfg, (3, 3, 2, 1)), PAIRS[:4]
    jobs = jobs_of(cfg, clips, pairs)
    q = open_queue(d, m, 2)
    try:
        a, b = q.submit(jobs[0]), q.submit(jobs[1], priority=1)
        assert q.run(1) == 1
        h, p = q.submit(jobs[2], priority=2), q.submit(jobs[3])
        q.park(p)
        assert q.run(1) == 1 and st(q, a) == (PARKED, -1, 1, 1, False) and st(q, p) == (PENDING, -1, 0, 0, True)
        q.park(b)
        assert q.info() == {"rounds_total": 2, "n_pending": 2, "n_running": 2}
    finally:
        q.close()
    used = _after(lib, cfg, m, d)
    assert len(fresh) == len(used) == 4 and all(np.array_equal(x, z) for x, z in zip(fresh, used))


def check_refusals(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """an unknown ticket: DSG_E_INVALID with the ticket in the message; a null queue"""
    mB, d = model(lib, cfg, prec, 1, kset), diffusion(lib)
    mB.set_schedule(d)
    s = RawSession(lib, [mB.handle], cfg, 1)
    assert s.rc == 0, s.msg
    try:
        assert s.submit(clips_of(cfg, (1,))[0], PAIRS[0]) == 0
        err = lambda: (lib.cdll.dsg_last_error() or b"").decode()
        for name, call in (("dsg_queue_set_priority", lambda t: lib.cdll.dsg_queue_set_priority(s.q, t, 1)),
                           ("dsg_queue_park", lambda t: lib.cdll.dsg_queue_park(s.q, t)),
                           ("dsg_queue_resume", lambda t: lib.cdll.dsg_queue_resume(s.q, t))):
            for t in (1, -1, 2 ** 40):
                assert call(t) == L.E_INVALID and f"{name}: no such ticket: {t}" in err(), (name, t, err())
            assert call(0) == 0
        assert lib.cdll.dsg_queue_set_priority(None, 0, 1) == L.E_INVALID and lib.cdll.dsg_queue_park(None, 0) == L.E_INVALID
        assert lib.cdll.dsg_queue_resume(None, 0) == L.E_INVALID
        assert s.run(0) == 1
    finally:
        s.close()
    with open_queue(d, mB, 1) as q:
        with pytest.raises(ValueError, match="no such ticket: 0"):
            q.park(0)


# ---- 10. the host plan ---------------------------------------------------------------------------------------------------------------------------
# Worked by hand: 2 slots; K, priority, the round before which each job is submitted.
#   round 0   waiting by (priority, ticket): 2, 0, 1, 3.  Slot 0 <- job 2, slot 1 <- job 0.  Jobs 1 and 3 find nobody placed before this round.
#   round 1   job 4 (prio 1) arrives; waiting: 4, 1, 3.  No slot is free.  Job 4: the running jobs are 2 (prio 1) and 0 (prio 0); the victim is
#             job 0, 0 < 1: job 0 is parked after one window and job 4 takes slot 1.  Job 1 (prio 0): the only job not placed in this round is
#             2 (prio 1), not lower: the placement ends.  Job 2 runs its last window.
#   round 2   slot 0 is free; waiting: 0 (parked), 1, 3 -- all prio 0, by ticket.  Job 0 resumes in slot 0 on window 1.  Job 4 runs its last.
#   round 3   slot 1 is free: job 1 takes it.  Job 0 runs its last window.
#   round 4   slot 0 is free: job 3 takes it and is done; job 1 runs its last window.
PLAN_K, PLAN_PRIO, PLAN_ARRIVE = (3, 2, 2, 1, 2), (0, 0, 1, 0, 1), (0, 0, 0, 0, 1)
PLAN_FIRST, PLAN_DONE, PLAN_PARKS, PLAN_ROUNDS = [0, 3, 0, 4, 1], [3, 4, 1, 4, 2], [1, 0, 0, 0, 0], 5


def check_place_prio(lib):
    assert L.queue_place_prio(PLAN_K, 2, PLAN_ARRIVE, PLAN_PRIO, lib) == (PLAN_FIRST, PLAN_DONE, PLAN_PARKS, PLAN_ROUNDS)
    rs = np.random.RandomState(2)
    for n_jobs, n_slots in ((48, 16), (7, 3), (3, 8), (1, 1), (20, 1)):
        K = rs.randint(1, 9, size=n_jobs)
        for arrive in (None, np.sort(rs.randint(0, 12, size=n_jobs))):
            slot, first, n_rounds = L.queue_place(K, n_slots, arrive, lib)
            for prio in (None, [-2] * n_jobs):
                f, done, parks, n = L.queue_place_prio(K, n_slots, arrive, prio, lib)
                assert (f, n) == (first, n_rounds) and parks == [0] * n_jobs and done == [a + int(k) - 1 for a, k in zip(first, K)]
            # with priorities: every job runs its K windows in K distinct rounds between its first and its last, whatever was parked
            f, done, parks, n = L.queue_place_prio(K, n_slots, arrive, rs.randint(0, 3, size=n_jobs), lib)
            assert all(done[j] - f[j] + 1 >= K[j] and f[j] >= (0 if arrive is None else arrive[j]) for j in range(n_jobs))
            assert n == max(done) + 1 and all(p >= 0 for p in parks)
            assert all(p == 0 for p, d_, f_, k in zip(parks, done, f, K) if d_ - f_ + 1 == k)
    one, r = np.ones(2, np.int32), ctypes.c_int32(0)
    P = lambda a: None if a is None else a.ctypes.data
    for K, arrive, n_jobs, n_slots, outs in (([0, 1], None, 2, 1, 4), ([1, 1], None, 2, 0, 4), ([1, 1], [2, 1], 2, 1, 4), ([1, 1], [-1, 1], 2, 1, 4),
                                             ([1, 1], None, 0, 1, 4), ([1, 1], None, 2, 1, 0), ([1, 1], None, 2, 1, 2), (None, None, 2, 1, 4)):
        k = None if K is None else np.array(K, np.int32)
        a = None if arrive is None else np.array(arrive, np.int32)
        o = [one.ctypes.data if i < outs else None for i in range(3)]
        rc = lib.cdll.dsg_queue_place_prio(P(k), P(a), None, n_jobs, n_slots, o[0], o[1], o[2], ctypes.byref(r) if outs == 4 else None)
        assert rc == L.E_INVALID, (K, arrive, n_jobs, n_slots, outs)
    with pytest.raises(ValueError, match="priority has 1 entries"):
        L.queue_place_prio([1, 2], 2, None, [0], lib)
    with pytest.raises(ValueError, match="arrive_round has 3 entries"):
        L.queue_place_prio([1, 2], 2, [0, 0, 0], None, lib)


# ---- 11. ABI -----------------------------------------------------------------------------------------------------------------------------------
def check_abi(lib):
    assert lib.cdll.dsg_version() == 330
    assert ctypes.sizeof(L.dsg_queue_job_info) == 32 and ctypes.sizeof(L.dsg_queue_window) == 32
    assert ctypes.sizeof(L.dsg_clip_job) == 80 and ctypes.sizeof(L.dsg_clip_edit) == 32
    assert [f[0] for f in L.dsg_queue_job_info._fields_] == ["state", "windows_done", "rows_ready", "slot", "first_round", "reserved"]
    for name in ("dsg_queue_set_priority", "dsg_queue_park", "dsg_queue_resume", "dsg_queue_place_prio"):
        assert name in L.SYMBOLS and hasattr(lib.cdll, name)
    assert (L.JOB_PARKED, L.JOB_HELD) == (4, 4) and (L.JOB_PENDING, L.JOB_RUNNING, L.JOB_DONE, L.JOB_CANCELLED) == (0, 1, 2, 3)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsg.h")).read()
    for decl in ("enum { DSG_JOB_PARKED = 4 };", "enum { DSG_JOB_HELD = 4 };", "int dsg_queue_set_priority(dsg_queue* q, int64_t ticket, int32_t priority);",
                 "int dsg_queue_park(dsg_queue* q, int64_t ticket);", "int dsg_queue_resume(dsg_queue* q, int64_t ticket);", "int dsg_queue_place_prio("):
        assert decl in header, decl


# ---- 12. the drivers of sample.py ------------------------------------------------------------------------------------------------------------
def check_drivers(lib, prec="bf16", kset="tile"):
    """`open_clip_queue` and `open_clip_queue_dsgplus` with `priority=`, `park` and `resume`: every clip is `generate_clip[_dsgplus](...,
    windows="library")` of the clip alone"""
    for cfg in (C.TINY, C.TINY5):
        mB, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
        Ks = (3, 1, 2)
        clips, ids = clips_of(cfg, Ks), [p[1] for p in PAIRS[:3]]
        root_shift, _ = layout(cfg)
        if _zeggs_like(cfg):
            dicts = [{"feats": c["feats"], "style": c["style"][0], "seed_pose": c["seed"], "clip_id": i} for c, i in zip(clips, ids)]
            opened = S.open_clip_queue(mB, d, seed=SHARED, skip_timesteps=SKIP, kernel_set=kset)
        else:
            dicts = [{"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"], "real_n_frames": K * cfg.stride - 3,
                      "clip_id": i} for c, K, i in zip(clips, Ks, ids)]
            opened = S.open_clip_queue_dsgplus(mB, d, seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=kset, B=1)
        with opened as q:
            a = q.submit(dicts[0])
            assert q.run(1) == 1
            h = q.submit(dict(dicts[1], priority=1))                                 # takes the only slot: a is parked
            assert q.run(1) == 1 and q.job(a)["state"] == PARKED and q.job(a)["parks"] == 1 and q.job(h)["state"] == DONE
            b = q.submit(dicts[2], priority=0)
            q.park(a)                                                                # the pause: b passes a
            assert q.run(0) == 2 and q.job(b)["state"] == DONE and q.job(a)["held"] and q.run(0) == 0
            q.resume(a)
            assert q.run(0) == 2 and q.job(a)["state"] == DONE
            q.set_priority(a, 2)
            got = [q.result(x) for x in (a, h, b)]
        for i in range(3):
            want = alone(cfg, m1, d, clips[i], (SHARED, ids[i]), root_shift=root_shift)
            want = want if _zeggs_like(cfg) else want[:Ks[i] * cfg.stride - 3]
            assert got[i].shape == want.shape and np.array_equal(got[i], want), (cfg.name, i)


# ---- GPU only ----------------------------------------------------------------------------------------------------------------------------------
def check_zeggs_rows(lib):
    """pre-emption at the ZEGGS widths, bf16, the ROWS set, B = 3 with jobs of K = 2, 3, 1 (as clip_queue_live_util.check_zeggs_rows): two
    prio-1 jobs arrive after round 0 -- one takes the slot job 2 left, the other parks job 1 (the highest ticket of the lowest priority),
    which comes back into slot 0: its rows leave and re-enter 16-row tiles shared with its neighbours"""
    cfg, B, Ks = C.ZEGGS, 3, (2, 3, 1, 1, 1)
    mB, m1, d = model(lib, cfg, "bf16", B, "rows"), model(lib, cfg, "bf16", 1, "rows"), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:5]
    jobs = jobs_of(cfg, clips, pairs)
    with open_queue(d, mB, B) as q:
        t = [q.submit(j) for j in jobs[:3]]
        assert q.run(1) == 1 and q.job(t[2])["state"] == DONE
        t += [q.submit(j, priority=1) for j in jobs[3:]]
        assert q.run(1) == 1
        assert st(q, t[1]) == (PARKED, -1, 1, 1, False) and st(q, t[0]) == (DONE, 0, 2, 0, False)
        assert [q.job(x)["slot"] for x in t[3:]] == [2, 1] and all(q.job(x)["state"] == DONE for x in t[3:])
        assert q.run(1) == 1 and st(q, t[1]) == (RUNNING, 0, 2, 1, False)
        assert q.run(0) == 1 and q.info() == {"rounds_total": 4, "n_pending": 0, "n_running": 0}
        got = [q.result(x) for x in t]
    assert mB.last_kernel_set() == "rows"
    assert L.queue_place_prio(Ks, B, (0, 0, 0, 1, 1), (0, 0, 0, 1, 1), lib) == ([0, 0, 0, 1, 1], [1, 3, 0, 1, 1], [0, 1, 0, 0, 0], 4)
    for i in range(5):
        want = alone(cfg, m1, d, clips[i], pairs[i])
        assert m1.last_kernel_set() == "rows"
        assert np.array_equal(got[i], want), (i, float(np.max(np.abs(got[i] - want))))


def check_beatpp_rows(lib):
    """the parity script at the BEAT++ widths (variant 5): y['seed_last'] follows the job into the new slot"""
    check_tail_parity(lib, C.BEATPP, "bf16", "rows", afters=(1, 2))


def check_device_pointers(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    """pre-emption (check 2) with every job tensor and `out` a device tensor that starts one float past a 16-byte boundary, two guard rows
    behind every `out`: the run equals the host-pointer run and the clips alone"""
    m, m1, d = model(lib, cfg, prec, 1, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    m.set_schedule(d)
    clips, pairs = clips_of(cfg, (4, 2)), PAIRS[:2]
    res = {}
    for device in (False, True):
        s = RawSession(lib, [m.handle], cfg, 1)
        assert s.rc == 0, s.msg
        try:
            a = s.submit(clips[0], pairs[0], device=device, offset=1 if device else 0)
            assert s.run(1, device) == 1
            h = s.submit(clips[1], pairs[1], device=device, offset=1 if device else 0)
            lib.check(lib.cdll.dsg_queue_set_priority(s.q, h, 1))
            assert s.run(1, device) == 1
            info = L.dsg_queue_job_info()
            lib.check(lib.cdll.dsg_queue_job(s.q, a, ctypes.byref(info)))
            assert (info.state, info.slot, info.windows_done, info.reserved[2]) == (PARKED, -1, 1, 1)
            assert s.run(0, device) == 4
            res[device] = [s.out(a), s.out(h)]
        finally:
            s.close()
    for i in range(2):
        assert np.array_equal(res[True][i], res[False][i]) and (res[True][i][-2:] == 7.0).all(), i
        assert np.array_equal(res[False][i][:-2], alone(cfg, m1, d, clips[i], pairs[i])), i
