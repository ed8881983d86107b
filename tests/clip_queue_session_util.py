"""Shared by tests/test_emu_clip_queue_session.py (CPU, the SIMT emulator) and tests/test_gpu_clip_queue_session.py (MI355X): the checks of
the clip queue as a session (dsg_queue_* / dsg_queue_place; `DSGDiffusion.open_clip_queue`, `sample.open_clip_queue[_dsgplus]`), written once
over a `DSGLibrary`.  Every comparison is `np.array_equal`: a clip out of the session against the same clip sampled alone on a batch-1 handle
through the existing clip drivers (`windows="library"`) with the same kernel set named on both sides.  All loops are four steps
(skip_timesteps = 996) unless a clip brings its own skip."""
import ctypes

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import lib as L
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.model import ClassifierFreeSampleModel
from tests import clip_queue_edit_util as E
from tests.clip_queue_edit_util import INIT, INP, NONE, edits_of
from tests.clip_queue_util import PAIRS, SHARED, SKIP, _after, accepted_sets, alone, clips_of, diffusion, model, n_out_of, queue_jobs, y_of   # noqa: F401

# the table of the issue: K, the session round before which each job is submitted, slots -> slot, first_round, n_rounds
KS_MAIN, ARRIVE_MAIN, SLOT_MAIN, FIRST_MAIN, ROUNDS_MAIN = (3, 1, 2, 1, 2), (0, 0, 1, 1, 2), (0, 1, 1, 0, 1), (0, 0, 1, 3, 3), 5
# the workload of tools/clip_queue_bench.py
K48 = (4, 2, 5, 16, 1, 2, 8, 2, 4, 12, 1, 8, 3, 1, 2, 5, 5, 2, 3, 2, 8, 5, 1, 12, 2, 3, 16, 16, 12, 1, 12, 12, 5, 1, 3, 1, 8, 2, 3, 5, 2, 8, 2, 12, 3,
       8, 16, 2)


# ---- 1. the placement (host only) -----------------------------------------------------------------------------------------------------------
def place_py(K, arrive, n_slots):
    """the rule, restated: at the start of every round the free slots, lowest first, take the jobs that have arrived, oldest first"""
    n = len(K)
    arrive = [0] * n if arrive is None else list(arrive)
    free_at, slot, first = [0] * n_slots, [0] * n, [0] * n
    nxt, r = 0, 0
    while nxt < n:
        if max(free_at) <= r and arrive[nxt] > r:
            r = arrive[nxt]
        for s in range(n_slots):
            if nxt < n and free_at[s] <= r and arrive[nxt] <= r:
                slot[nxt], first[nxt] = s, r
                free_at[s] = r + K[nxt]
                nxt += 1
        r += 1
    return slot, first, max(free_at)


def check_place(lib):
    assert L.queue_place(KS_MAIN, 2, ARRIVE_MAIN, lib) == (list(SLOT_MAIN), list(FIRST_MAIN), ROUNDS_MAIN)
    assert sum(K48) == 269
    assert L.queue_place(K48, 16, None, lib)[2] == 26                               # index order
    assert L.queue_place(sorted(K48, reverse=True), 16, None, lib)[2] == 17         # longest first: the one-shot plan's rounds
    assert L.queue_place(sorted(K48, reverse=True), 16, None, lib)[2] == L.clip_queue_plan(K48, 16, lib)[2]
    slot, first, n_rounds = L.queue_place(K48, 16, [0] * 47 + [3], lib)             # the last job (K = 2) arrives before round 3
    assert K48[47] == 2 and (slot[47], first[47], n_rounds) == (7, 11, 26)
    rs = np.random.RandomState(1)
    for n_jobs, n_slots in ((48, 16), (7, 3), (3, 8), (1, 1), (20, 1)):
        K = rs.randint(1, 9, size=n_jobs)
        for arrive in (None, np.sort(rs.randint(0, 12, size=n_jobs))):
            slot, first, n_rounds = L.queue_place(K, n_slots, arrive, lib)
            assert (slot, first, n_rounds) == place_py(list(K), arrive, n_slots), (n_jobs, n_slots)
            busy = np.zeros((n_slots, n_rounds), int)
            for j in range(n_jobs):
                assert 0 <= slot[j] < n_slots and first[j] >= (0 if arrive is None else arrive[j]) and first[j] + K[j] <= n_rounds
                busy[slot[j], first[j]:first[j] + K[j]] += 1
            assert busy.max() == 1                                                  # no two jobs overlap in a slot
            assert all(first[j] <= first[j + 1] for j in range(n_jobs - 1))         # first come, first served
    one, r = np.ones(2, np.int32), ctypes.c_int32(0)
    for K, arrive, n_jobs, n_slots in (([0, 1], None, 2, 1), ([1, 1], None, 2, 0), ([1, 1], [2, 1], 2, 1), ([1, 1], None, 0, 1)):
        k = np.array(K, np.int32)
        a = None if arrive is None else np.array(arrive, np.int32)
        rc = lib.cdll.dsg_queue_place(k.ctypes.data, None if a is None else a.ctypes.data, n_jobs, n_slots, one.ctypes.data, one.ctypes.data,
                                      ctypes.byref(r))
        assert rc == L.E_INVALID, (K, arrive, n_jobs, n_slots)
    with pytest.raises(ValueError, match="arrive_round has 1 entries"):
        L.queue_place([1, 2], 2, [0], lib)


# ---- the session ------------------------------------------------------------------------------------------------------------------------------
def open_queue(d, lanes, B, ddim=False, root_shift=True, keep_last_tail=False, guided=False, skip=SKIP):
    d.manual_seed(SHARED, 99)
    return d.open_clip_queue(lanes, B, root_shift=root_shift, keep_last_tail=keep_last_tail, ddim=ddim, eta=0.5, skip_timesteps=skip, guided=guided)


def rows_ready_of(cfg, K, windows_done, keep_last_tail):
    n_out = n_out_of(cfg, K, keep_last_tail)
    if windows_done >= K:
        return n_out
    # (window c leaves rows [c * stride - n_seed, (c + 1) * stride - n_seed) final; with keep_last_tail only the last window writes its tail)
    return max(0, min(n_out, windows_done * cfg.stride - cfg.n_seed))


def expect_job(cfg, K, slot, first, submitted, rounds_done, keep_last_tail=False):
    """what dsg_queue_job reports for a job of the placement (slot, first) once `rounds_done` rounds of the session have run"""
    if not submitted or first >= rounds_done:
        return {"state": L.JOB_PENDING, "windows_done": 0, "rows_ready": 0, "slot": -1, "first_round": -1}
    w = min(K, rounds_done - first)
    return {"state": L.JOB_DONE if w == K else L.JOB_RUNNING, "windows_done": w, "rows_ready": rows_ready_of(cfg, K, w, keep_last_tail), "slot": slot,
            "first_round": first}


def run_arrivals(q, jobs, arrive, outs=None, each_round=None):
    """submit jobs[j] before session round arrive[j], one round per `run(1)` up to the last instalment, then `run(0)`; `each_round(rounds
    done, tickets so far)` after every run.  Returns the tickets"""
    tickets, r = [], 0
    last = max(arrive)
    while True:
        for j in range(len(jobs)):
            if arrive[j] == r:
                tickets.append(q.submit(jobs[j], out=None if outs is None else outs[j]))
        if r < last:
            assert q.run(1) == 1
            r += 1
            if each_round:
                each_round(r, tickets)
            continue
        n = q.run(0)
        if each_round:
            each_round(r + n, tickets)
        assert q.run(0) == 0 and q.run(1) == 0                                       # idle: nothing alive, nothing pending
        return tickets


# ---- 2. arrivals: every clip equals the clip alone, the table round by round ------------------------------------------------------------------
def check_arrivals(lib, cfg, prec, kset, combos=((False, True), (True, False)), B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, KS_MAIN), PAIRS[:len(KS_MAIN)]
    jobs = queue_jobs(cfg, clips, pairs)
    for ddim, root_shift in combos:
        with open_queue(d, mB, B, ddim=ddim, root_shift=root_shift) as q:
            def table(rounds_done, tickets, q=q):
                for j in range(len(KS_MAIN)):
                    want = expect_job(cfg, KS_MAIN[j], SLOT_MAIN[j], FIRST_MAIN[j], j < len(tickets), rounds_done)
                    if j < len(tickets):
                        assert q.job(tickets[j]) == want, (rounds_done, j, q.job(tickets[j]), want)
                assert q.info()["rounds_total"] == min(rounds_done, ROUNDS_MAIN)
            tickets = run_arrivals(q, jobs, ARRIVE_MAIN, each_round=table)
            assert tickets == list(range(5)) and q.info() == {"rounds_total": ROUNDS_MAIN, "n_pending": 0, "n_running": 0}
            assert mB.last_sample_ms()[1] == 3 * 4                                   # the last run call: three rounds of four steps
            got = [q.result(t) for t in tickets]
            with pytest.raises(ValueError, match="no such ticket"):
                q.job(5)
        assert mB.last_kernel_set() == kset and d._draw == max(KS_MAIN) * 5
        for i, (clip, pair) in enumerate(zip(clips, pairs)):
            want = alone(cfg, m1, d, clip, pair, ddim=ddim, root_shift=root_shift)
            assert m1.last_kernel_set() == kset
            assert got[i].shape == want.shape == (n_out_of(cfg, KS_MAIN[i], False), cfg.njoints)
            assert np.array_equal(got[i], want), (cfg.name, prec, kset, ddim, root_shift, i, float(np.max(np.abs(got[i] - want))))


# ---- 3. per-window delivery ---------------------------------------------------------------------------------------------------------------
def _dsgplus_jobs(cfg, clips, pairs, scales=None):
    """the dicts of `open_clip_queue` for the DSG+ layout: the per-window features as `_dsgplus_window_y` builds them"""
    jobs = []
    for i, (c, p) in enumerate(zip(clips, pairs)):
        audio = [S._dsgplus_window_y(cfg, list(c["feats"]), w, None, c["seed"], c["seed_last"], False, None)["audio"] for w in range(len(c["feats"]))]
        jobs.append({"feats": audio, "style": c["style"], "seed0": c["seed"], "seed_last": c["seed_last"], "stream": p,
                     "scale": None if scales is None else scales[i]})
    return jobs


def check_delivery(lib, cfg, keep_last_tail, prec="bf16", kset="tile", B=2):
    """host `out`s filled with 7.0: after every round rows [0, rows_ready) are the finished clip's, everything behind is still 7.0"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, KS_MAIN), PAIRS[:len(KS_MAIN)]
    jobs = _dsgplus_jobs(cfg, clips, pairs) if keep_last_tail else queue_jobs(cfg, clips, pairs)
    want = [alone(cfg, m1, d, c, p, root_shift=not keep_last_tail) for c, p in zip(clips, pairs)]
    outs = [np.full((n_out_of(cfg, K, keep_last_tail), cfg.njoints), 7.0, np.float32) for K in KS_MAIN]
    seen = []

    def rows(rounds_done, tickets):
        for j, out in enumerate(outs):
            e = expect_job(cfg, KS_MAIN[j], SLOT_MAIN[j], FIRST_MAIN[j], j < len(tickets), rounds_done, keep_last_tail)
            n = e["rows_ready"]
            if j < len(tickets):
                assert q.job(tickets[j])["rows_ready"] == n and q.rows(tickets[j]).shape == (n, cfg.njoints)
            assert np.array_equal(out[:n], want[j][:n]) and (out[n:] == 7.0).all(), (rounds_done, j, n)
        seen.append([expect_job(cfg, K, s, f, True, rounds_done, keep_last_tail)["rows_ready"] for K, s, f in zip(KS_MAIN, SLOT_MAIN, FIRST_MAIN)])

    with open_queue(d, mB, B, root_shift=not keep_last_tail, keep_last_tail=keep_last_tail) as q:
        rows(0, [])
        run_arrivals(q, jobs, ARRIVE_MAIN, outs=outs, each_round=rows)
    # (job 0, K = 3: a first window delivers stride - n_seed rows; partial rows were really seen)
    assert seen[1][0] == cfg.stride - cfg.n_seed and 0 < seen[2][0] < outs[0].shape[0]
    for out, w in zip(outs, want):
        assert np.array_equal(out, w)


# ---- the raw exports ------------------------------------------------------------------------------------------------------------------------
class RawSession:
    """dsg_queue_* through ctypes alone.  `device`: every tensor of a job as a torch device tensor that starts `offset` floats (bytes for
    the mask) past an allocation's start"""

    def __init__(self, lib, handles, cfg, B, keep_last_tail=0, root_shift=1, skip=SKIP, guided=0):
        self.lib, self.cfg, self.keep_last_tail = lib, cfg, keep_last_tail
        a = L.dsg_sample_args()
        a.mode, a.skip_timesteps = L.MODE_DDPM, skip
        hs = (ctypes.c_void_p * len(handles))(*handles)
        self.q = ctypes.c_void_p()
        ones = np.ones(cfg.n_poses, np.uint8)
        self.rc = lib.cdll.dsg_queue_open(hs, len(handles), B, ones.ctypes.data, guided, ctypes.byref(a), root_shift, keep_last_tail, ctypes.byref(self.q))
        self.msg = (lib.cdll.dsg_last_error() or b"").decode()
        self.keep, self.outs, self.host = [], [], []

    def submit(self, clip, pair, edit=None, skip=-1, device=False, offset=0, guard=2, audio=None):
        """returns the ticket; the job's host arrays are kept in self.host[ticket] (style, seed0, audio, edit tensors)"""
        cfg = self.cfg
        K = len(clip["feats"])
        audio = np.ascontiguousarray(np.concatenate(clip["feats"] if audio is None else audio), np.float32)
        arrays = {"style": np.array(clip["style"], np.float32), "seed0": np.array(clip["seed"], np.float32), "audio": audio}
        if clip.get("seed_last") is not None:
            arrays["seed_last"] = np.array(clip["seed_last"], np.float32)
        for key, field in (("inpainting_mask", "inp_mask"), ("inpainted_motion", "inp_motion"), ("init_motion", "init_motion")):
            if edit and key in edit:
                arrays[field] = np.array(edit[key])
        out = np.full((n_out_of(cfg, K, self.keep_last_tail) + guard, cfg.njoints), 7.0, np.float32)
        if device:
            import torch

            def dev(a):
                flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
                flat[offset:] = torch.from_numpy(a.reshape(-1)).cuda()
                return flat[offset:]
            tensors = {k: dev(v) for k, v in arrays.items()}
            out = dev(out).view(out.shape)
            ptr = lambda t: t.data_ptr()
            assert all(ptr(t) % 16 == (offset * t.element_size()) % 16 for t in tensors.values())
        else:
            tensors, ptr = arrays, lambda a: a.ctypes.data
        job, ed = L.dsg_clip_job(), L.dsg_clip_edit()
        job.style, job.seed0, job.audio, job.out = ptr(tensors["style"]), ptr(tensors["seed0"]), ptr(tensors["audio"]), ptr(out)
        if "seed_last" in tensors:
            job.seed_last = ptr(tensors["seed_last"])
        job.K, job.scale, job.seed, job.stream_id = K, 1.0, pair[0], pair[1]
        for field in ("inp_mask", "inp_motion", "init_motion"):
            if field in tensors:
                setattr(ed, field, ptr(tensors[field]))
        t = ctypes.c_int64(-1)
        stream = L.current_stream_ptr() if device else None
        self.lib.check(self.lib.cdll.dsg_queue_submit(self.q, ctypes.byref(job), ctypes.byref(ed) if edit else None, skip, ctypes.byref(t), stream))
        self.keep.append(tensors)
        self.outs.append(out)
        self.host.append(arrays)
        return int(t.value)

    def run(self, max_rounds, device=False):
        n = ctypes.c_int(-1)
        self.lib.check(self.lib.cdll.dsg_queue_run(self.q, max_rounds, ctypes.byref(n), L.current_stream_ptr() if device else None))
        return int(n.value)

    def out(self, t):
        o = self.outs[t]
        if L.is_torch(o):
            import torch
            torch.cuda.synchronize()
            return o.cpu().numpy()
        return o

    def close(self):
        if self.q:
            self.lib.check(self.lib.cdll.dsg_queue_close(self.q))
            self.q = None


# ---- 4. inputs are free after submit ----------------------------------------------------------------------------------------------------------
def check_inputs_free(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 2), kinds=(INP | INIT, NONE, INIT), B=2):
    """every host tensor of a job -- style, seed0, audio, the three edit tensors -- overwritten right after dsg_queue_submit (NaN; the mask
    with 0xff): the result is the clip alone with the tensors as they were"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    mB.set_schedule(d)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    s = RawSession(lib, [mB.handle], cfg, B)
    assert s.rc == 0, s.msg
    try:
        for i in range(len(Ks)):
            t = s.submit(clips[i], pairs[i], edits[i])
            assert t == i
            for a in s.host[t].values():
                a.fill(0xff if a.dtype == np.uint8 else np.nan)
            if i == 0:
                assert s.run(1) == 1
        assert s.run(0) == 3
        for i in range(len(Ks)):
            want = E.alone(cfg, m1, d, clips[i], pairs[i], edits[i])
            got = s.out(i)
            assert np.array_equal(got[:-2], want) and (got[-2:] == 7.0).all(), i
    finally:
        s.close()


# ---- 5. edits and strengths arriving late ---------------------------------------------------------------------------------------------------
def check_late_edits(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 2, 2), kinds=(NONE, INIT, INP), skips=(996, 998, 999), B=2,
                     combos=((False, True), (True, False))):
    """a fresh clip, an init-motion edit and an inpainted clip, one more per round: holds of 2 and 1 beside a neighbour on its second
    window, and a last round that runs the single last step"""
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, False, kinds)
    jobs = [dict(j, **e, **({} if s == SKIP else {"skip_timesteps": s})) for j, e, s in zip(queue_jobs(cfg, clips, pairs), edits, skips)]
    for ddim, root_shift in combos:
        with open_queue(d, mB, B, ddim=ddim, root_shift=root_shift) as q:
            tickets = run_arrivals(q, jobs, (0, 1, 2))
            assert q.info()["rounds_total"] == 4 and [q.job(t)["first_round"] for t in tickets] == [0, 1, 2]
            assert mB.last_sample_ms()[1] == 2 + 1                                   # run(0): a round from skip 998, a round from 999
            got = [q.result(t) for t in tickets]
        assert not mB.inpainting and mB.noise_streams is None
        assert d._draw == max(K * (1 + d.num_timesteps - s) for K, s in zip(Ks, skips))
        for i in range(len(Ks)):
            want = E.alone(cfg, m1, d, clips[i], pairs[i], edits[i], ddim=ddim, root_shift=root_shift, skip=skips[i])
            assert np.array_equal(got[i], want), (ddim, root_shift, i, float(np.max(np.abs(got[i] - want))))


# ---- 6. cancel ---------------------------------------------------------------------------------------------------------------------------------
def check_cancel(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(3, 2, 1, 2, 1), B=2):
    mB, m1, d = model(lib, cfg, prec, B, kset), model(lib, cfg, prec, 1, kset), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    jobs = queue_jobs(cfg, clips, pairs)
    want = [alone(cfg, m1, d, c, p) for c, p in zip(clips, pairs)]
    outs = [np.full((n_out_of(cfg, K, False), cfg.njoints), 7.0, np.float32) for K in Ks]
    with open_queue(d, mB, B) as q:
        t = [q.submit(j, out=o) for j, o in zip(jobs, outs)]
        q.cancel(t[4])                                                               # pending: it never gets a slot
        assert q.info() == {"rounds_total": 0, "n_pending": 4, "n_running": 0}
        assert q.run(1) == 1
        n1 = rows_ready_of(cfg, Ks[1], 1, False)
        assert q.job(t[1]) == {"state": L.JOB_RUNNING, "windows_done": 1, "rows_ready": n1, "slot": 1, "first_round": 0}
        q.cancel(t[1])                                                               # after its first window
        q.cancel(t[1])                                                               # (again: nothing left to cancel)
        assert q.job(t[1]) == {"state": L.JOB_CANCELLED, "windows_done": 1, "rows_ready": n1, "slot": 1, "first_round": 0}
        assert q.info() == {"rounds_total": 1, "n_pending": 2, "n_running": 1}
        with pytest.raises(L.DSGError, match="not done"):
            q.result(t[1])
        assert q.run(1) == 1
        assert q.job(t[2])["slot"] == 1 and q.job(t[2])["first_round"] == 1          # the next ticket took the slot in the following round
        assert q.run(0) == 2                                                         # job 0's last window, then job 3's second
        assert q.job(t[3]) == {"state": L.JOB_DONE, "windows_done": 2, "rows_ready": outs[3].shape[0], "slot": 1, "first_round": 2}
        assert q.job(t[4]) == {"state": L.JOB_CANCELLED, "windows_done": 0, "rows_ready": 0, "slot": -1, "first_round": -1}
        q.cancel(t[0])                                                               # done already: a no-op
        assert q.job(t[0])["state"] == L.JOB_DONE and q.info() == {"rounds_total": 4, "n_pending": 0, "n_running": 0}
    assert 0 < n1 < outs[1].shape[0]
    assert np.array_equal(outs[1][:n1], want[1][:n1]) and (outs[1][n1:] == 7.0).all()      # exactly the rows of its first window
    assert (outs[4] == 7.0).all()
    for i in (0, 2, 3):
        assert np.array_equal(outs[i], want[i]), i


# ---- 7. lanes ---------------------------------------------------------------------------------------------------------------------------------
def check_lanes(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3, 1, 1, 2), arrive=(0, 0, 0, 1, 1, 2)):
    d = diffusion(lib)
    base = model(lib, cfg, prec, 4, kset)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    jobs = queue_jobs(cfg, clips, pairs)
    slot, first, n_rounds = L.queue_place(Ks, 4, arrive, lib)
    per = {}
    for n_lanes, B in ((2, 2), (1, 4), (4, 1)):
        lanes = [base] + [base.clone(B) for _ in range(n_lanes - 1)]
        with open_queue(d, lanes, B) as q:
            tickets = run_arrivals(q, jobs, arrive)
            assert q.info()["rounds_total"] == n_rounds
            assert [(q.job(t)["slot"], q.job(t)["first_round"]) for t in tickets] == list(zip(slot, first))
            per[n_lanes] = [q.result(t) for t in tickets]
        assert all(ln.last_kernel_set() == kset and ln.noise_streams is None for ln in lanes)
    for i in range(len(Ks)):
        assert np.array_equal(per[2][i], per[1][i]) and np.array_equal(per[2][i], per[4][i]), i
    assert len({g.tobytes() for g in per[2]}) == len(Ks)
    m1 = model(lib, cfg, prec, 1, kset)
    for i in (2, 5):
        assert np.array_equal(per[2][i], alone(cfg, m1, d, clips[i], pairs[i])), i


# ---- 8. guidance and variant 5, through the DSG+ driver ------------------------------------------------------------------------------------
def check_guided_v5(lib, cfg=C.TINY5, prec="bf16", kset="tile", Ks=(2, 1, 2), scales=(2.5, 1.0, 0.5), B=2):
    mB, m1, d = model(lib, cfg, prec, 2 * B, kset), model(lib, cfg, prec, 2, kset), diffusion(lib)
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:len(Ks)]]
    real = [K * cfg.stride - 3 * i for i, K in enumerate(Ks)]
    dicts = [{"feats": c["feats"], "style": c["style"], "seed_pose": c["seed"], "seed_last": c["seed_last"], "real_n_frames": r, "clip_id": i, "scale": s}
             for c, r, i, s in zip(clips, real, ids, scales)]
    with S.open_clip_queue_dsgplus(ClassifierFreeSampleModel(mB), d, seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=None, B=B) as q:
        t = [q.submit(dicts[0]), q.submit(dicts[1])]
        assert q.run(1) == 1
        assert q.rows(t[0]).shape == (cfg.stride - cfg.n_seed, cfg.njoints) and q.result(t[1]).shape == (real[1], cfg.njoints)
        t.append(q.submit(dicts[2]))                                                 # takes slot 1 in round 1
        assert q.run(0) == 2 and q.job(t[2])["slot"] == 1 and q.job(t[2])["first_round"] == 1
        got = [q.result(x) for x in t]
    assert mB.last_kernel_set() == kset
    for i, (clip, sid) in enumerate(zip(clips, ids)):
        audio = [S._dsgplus_window_y(cfg, list(clip["feats"]), w, None, clip["seed"], clip["seed_last"], False, None)["audio"] for w in range(Ks[i])]
        d.manual_seed(SHARED, sid)
        want = d.sample_clip(ClassifierFreeSampleModel(m1), audio, clip["style"], seed0=clip["seed"], root_shift=False, keep_last_tail=True,
                             skip_timesteps=SKIP, scale=np.array([scales[i]], np.float32), seed_last=clip["seed_last"])[0][:real[i]]
        assert m1.last_kernel_set() == kset
        assert got[i].shape == (real[i], cfg.njoints) and np.array_equal(got[i], want), (cfg.name, i, float(np.max(np.abs(got[i] - want))))
    assert not np.array_equal(got[0], got[2])


def check_zeggs_driver(lib, cfg=C.TINY, prec="bf16", kset="tile", Ks=(2, 1, 3)):
    """`sample.open_clip_queue`: one seed, clip ids; the kernel set named at open is put back at close"""
    m1, d = model(lib, cfg, prec, 1, kset), diffusion(lib)
    mB = None
    for other in ("block", "stream", "latency"):       # the lane comes with another set than the session's
        try:
            mB = model(lib, cfg, prec, 2, other)
            break
        except (NotImplementedError, ValueError):
            continue
    assert mB is not None
    clips = clips_of(cfg, Ks)
    ids = [p[1] for p in PAIRS[:3]]
    with S.open_clip_queue(mB, d, seed=SHARED, skip_timesteps=SKIP, kernel_set=kset) as q:
        with pytest.raises(L.DSGError, match="belongs to an open queue"):
            mB.set_kernel_set(other)
        t = [q.submit({"feats": c["feats"], "style": c["style"][0], "seed_pose": c["seed"], "clip_id": i}) for c, i in zip(clips, ids)]
        assert q.run(0) == 4
        got = [q.result(x) for x in t]
    assert mB.last_kernel_set() == kset and mB.kernel_set() == other
    for i in range(3):
        assert np.array_equal(got[i], alone(cfg, m1, d, clips[i], (SHARED, ids[i]))), i


# ---- 9. ownership, and nothing sticks ---------------------------------------------------------------------------------------------------------
def check_ownership(lib, cfg=C.TINY, prec="bf16", kset="tile"):
    d = diffusion(lib)
    fresh = _after(lib, cfg, model(lib, cfg, prec, 2, kset), d)
    m = model(lib, cfg, prec, 2, kset)
    lane = m.clone(2)
    clips, pairs = clips_of(cfg, KS_MAIN), PAIRS[:5]
    jobs = queue_jobs(cfg, clips, pairs)
    y = y_of(cfg, (10, 11))
    shape = (2, cfg.njoints, 1, cfg.n_poses)
    buf = np.zeros(shape, np.float32)
    a = L.dsg_sample_args()
    a.mode, a.skip_timesteps = L.MODE_DDPM, SKIP
    q = open_queue(d, [m, lane], 1)
    try:
        for t in range(3):
            q.submit(jobs[t])
        assert q.run(1) == 1
        for h in (m.handle, lane.handle):
            calls = (lambda: lib.cdll.dsg_sample(h, ctypes.byref(a), buf.ctypes.data, 2, None),
                     lambda: lib.cdll.dsg_set_window_cond(h, y["style"].ctypes.data, y["seed"].ctypes.data, y["audio"].ctypes.data, None, 1, 2, 0, None),
                     lambda: lib.cdll.dsg_set_kernel_set(h, L.KERNEL_SETS["tile"]),
                     lambda: lib.cdll.dsg_set_noise_streams(h, None, None, 0),
                     lambda: lib.cdll.dsg_destroy(h))
            for call in calls:
                assert call() == L.E_STATE and b"handle belongs to an open queue" in lib.cdll.dsg_last_error()
        # a second session on a lane of an open one is refused; the lanes can still be cloned, synchronised and asked
        with pytest.raises(L.DSGError, match="belongs to an open queue"):
            open_queue(d, lane, 1)
        assert m.clone(1).max_batch == 1 and m.kernel_set() == kset and m.last_kernel_set() == kset and m.last_sample_ms()[1] == 4
        lib.check(lib.cdll.dsg_sync(m.handle))
        assert q.run(1) == 1                                                         # the refusals changed nothing: the session goes on
        assert q.job(0)["state"] == L.JOB_RUNNING and q.job(2)["state"] == L.JOB_RUNNING
    finally:
        q.close()                                                                    # with job 0 running (window 2 of 3) and job 2 too
    q.close()
    with pytest.raises(L.DSGError, match="closed"):
        q.run(1)
    assert m.noise_streams is None and not m.inpainting
    for h in (m, lane):
        used = _after(lib, cfg, h, d)
        assert len(fresh) == len(used) == 4 and all(np.array_equal(x, z) for x, z in zip(fresh, used))
    # and a session opens again on the same lanes
    m1 = model(lib, cfg, prec, 1, kset)
    with open_queue(d, [m, lane], 1) as q2:
        t = q2.submit(jobs[3])
        assert q2.run(0) == 1
        assert np.array_equal(q2.result(t), alone(cfg, m1, d, clips[3], pairs[3]))


def check_open_refusals(lib, cfg=C.TINY, prec="fp32", kset="tile"):
    """the refusals of dsg_sample_clip_queue_steps on lanes, B, guided and args, with its messages; a job's with its ticket"""
    d = diffusion(lib)
    m = model(lib, cfg, prec, 2, kset)
    m.set_schedule(d)
    clips = clips_of(cfg, (2, 1))
    for kw, match in ((dict(B=0), "B < 1"), (dict(B=3), "exceeds max_batch"), (dict(B=2, guided=1), "max_batch >= 2 * B")):
        s = RawSession(lib, [m.handle], cfg, kw.pop("B"), **kw)
        assert s.rc == L.E_INVALID and match in s.msg, (s.rc, s.msg)
    s = RawSession(lib, [m.handle, m.handle], cfg, 1)
    assert s.rc == L.E_INVALID and "appears twice" in s.msg
    s = RawSession(lib, [m.handle], cfg, 2, skip=1000)
    assert s.rc == L.E_INVALID and "skip_timesteps" in s.msg
    m.set_noise_streams(None, [1, 2])
    s = RawSession(lib, [m.handle], cfg, 2)
    assert s.rc == L.E_INVALID and "noise streams" in s.msg
    m.set_noise_streams(None, None)
    from diffusestylegesture_amd.model import DSGDenoiser
    raw = DSGDenoiser(cfg, precision=prec, max_batch=2, library=lib)
    s = RawSession(lib, [raw.handle], cfg, 2)
    assert s.rc == L.E_STATE and "dsg_finalize_weights" in s.msg
    s = RawSession(lib, [m.handle], cfg, 2)
    assert s.rc == 0, s.msg
    try:
        assert s.submit(clips[0], PAIRS[0]) == 0
        for bad, match in ((dict(skip=1000), "job 1 has skip_timesteps 1000"), (dict(edit={"inpainted_motion": np.zeros((14, cfg.njoints), np.float32)}), "job 1 has one of them")):
            with pytest.raises(ValueError, match=match):
                s.submit(clips[1], PAIRS[1], **bad)
        assert s.submit(clips[1], PAIRS[1]) == 1 and s.run(0) == 2                   # a refused submit takes no ticket
    finally:
        s.close()


# ---- 10. ABI -----------------------------------------------------------------------------------------------------------------------------------
def check_abi(lib):
    assert lib.cdll.dsg_version() == 330
    assert ctypes.sizeof(L.dsg_queue_job_info) == 32 and ctypes.sizeof(L.dsg_clip_job) == 80 and ctypes.sizeof(L.dsg_clip_edit) == 32
    for name in ("dsg_queue_open", "dsg_queue_submit", "dsg_queue_run", "dsg_queue_job", "dsg_queue_info", "dsg_queue_cancel", "dsg_queue_close",
                 "dsg_queue_place"):
        assert name in L.SYMBOLS and hasattr(lib.cdll, name)
    assert (L.JOB_PENDING, L.JOB_RUNNING, L.JOB_DONE, L.JOB_CANCELLED) == (0, 1, 2, 3)
    assert lib.cdll.dsg_queue_close(None) == 0


# ---- 11. GPU only ------------------------------------------------------------------------------------------------------------------------------
def check_zeggs_rows(lib):
    """ZEGGS widths, bf16, the ROWS set, B = 3: the last two clips arrive after round 0"""
    cfg, Ks, B = C.ZEGGS, (2, 1, 1, 1), 3
    mB, m1, d = model(lib, cfg, "bf16", B, "rows"), model(lib, cfg, "bf16", 1, "rows"), diffusion(lib)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:4]
    with open_queue(d, mB, B) as q:
        tickets = run_arrivals(q, queue_jobs(cfg, clips, pairs), (0, 0, 1, 1))
        assert q.info()["rounds_total"] == 2 and [q.job(t)["slot"] for t in tickets] == [0, 1, 1, 2]
        got = [q.result(t) for t in tickets]
    assert mB.last_kernel_set() == "rows"
    for i in range(4):
        want = alone(cfg, m1, d, clips[i], pairs[i])
        assert m1.last_kernel_set() == "rows"
        assert np.array_equal(got[i], want), (i, float(np.max(np.abs(got[i] - want))))


def check_device_pointers(lib, cfg, keep_last_tail, prec="bf16", kset="tile", Ks=(2, 1, 3), kinds=(INP, INIT, NONE), B=2):
    """every pointer of a job a device tensor that starts one float past a 16-byte boundary: the 4-byte path of the gather (and of the
    hand-off's stores) beside the 16-byte path of the staged run; two guard rows behind every `out`"""
    m, d = model(lib, cfg, prec, B, kset), diffusion(lib)
    m.set_schedule(d)
    clips, pairs = clips_of(cfg, Ks), PAIRS[:len(Ks)]
    edits = edits_of(cfg, Ks, keep_last_tail, kinds)
    audio = [None] * len(Ks) if not keep_last_tail else [j["feats"] for j in _dsgplus_jobs(cfg, clips, pairs)]
    res = {}
    for device in (False, True):
        s = RawSession(lib, [m.handle], cfg, B, keep_last_tail=int(keep_last_tail), root_shift=int(not keep_last_tail))
        assert s.rc == 0, s.msg
        try:
            for i in range(len(Ks)):
                s.submit(clips[i], pairs[i], edits[i], device=device, offset=1 if device else 0, audio=audio[i])
                if i == 1:
                    assert s.run(1, device) == 1
            assert s.run(0, device) == 3
            res[device] = [s.out(i) for i in range(len(Ks))]
        finally:
            s.close()
    m1 = model(lib, cfg, prec, 1, kset)
    for i in range(len(Ks)):
        assert np.array_equal(res[True][i], res[False][i]) and (res[True][i][-2:] == 7.0).all(), i
    for i in range(len(Ks)):
        assert np.array_equal(res[False][i][:-2], E.alone(cfg, m1, d, clips[i], pairs[i], edits[i])), i
