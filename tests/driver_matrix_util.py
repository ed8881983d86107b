"""Shared by tests/test_emu_driver_matrix.py (CPU, the SIMT emulator) and tests/test_gpu_driver_matrix.py (MI355X): the clip drivers of
sample.py with their options TOGETHER -- `clip_ids`, a clip-level constraint, an init motion, a seed pose, a second lane, a lane whose
per-lane entries are None -- where the other files pin each option alone.  Written once over a `DSGLibrary`.  Every comparison is
`np.array_equal`: the host window loop against the library's (`windows="host"` / `"library"`), and every clip against `generate_clip[_dsgplus]`
of that clip alone on a batch-1 lane with `stream_id` = its clip id and its own edits, under the same named kernel set.  bf16, the "tile"
set, four steps per window; feature_division = 1 and real_n_frames = K * stride, so every frame is compared."""
import numpy as np

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd import sample as S
from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
from diffusestylegesture_amd.synth import synth_window_inputs
from tests.clip_init_util import clip_init
from tests.clip_inpaint_util import clip_constraint, n_out_of
from tests.clip_queue_util import clips_of
from tests.noise_streams_util import SHARED, SKIP, _clip_inputs, diffusion, model

PREC, KSET = "bf16", "tile"
CLIP_IDS = [[7, 3], [5, 9]]            # per lane, per slot
CLIPS = [[10, 11], [12, 13]]           # the conditioning of the same four clips
SAMPLE_FN_KEYWORDS = {"clip_denoised", "model_kwargs", "skip_timesteps", "init_image", "progress", "dump_steps", "noise", "const_noise"}


def _zeggs(cfg):
    return cfg is C.TINY


def _lane_inputs(cfg, clips, K):
    """(feats, style, seed pose, seed_last or None) of the B clips of one lane"""
    feats, style, seed = _clip_inputs(cfg, clips, K)
    return feats, style, seed, synth_window_inputs(cfg, len(clips), window=0, clips=list(clips)).get("seed_last")


def _edits(cfg, B, K):
    """a clip-level constraint and an init motion for the B clips of one lane"""
    klt = not _zeggs(cfg)
    mask, motion, _ = clip_constraint(cfg, B, K, klt)
    return {"inpainting_mask": mask, "inpainted_motion": motion, "init_motion": clip_init(cfg, B, K, klt)}


def _row(ins, edits, b):
    """clip b of a lane as a batch of one"""
    feats, style, seed, last = ins
    return ([f[b:b + 1] for f in feats], style[b:b + 1], seed[b:b + 1], None if last is None else last[b:b + 1]), \
        {k: v[b:b + 1] for k, v in edits.items()}


def _single(cfg, m, d, ins, windows, skip=SKIP, seed_pose=True, **kw):
    """`generate_clip` / `generate_clip_dsgplus` of one lane"""
    feats, style, seed, last = ins
    if _zeggs(cfg):
        return S.generate_clip(m, d, feats, style, seed=SHARED, skip_timesteps=skip, seed_pose=seed if seed_pose else None, windows=windows, **kw)
    return S.generate_clip_dsgplus(m, d, feats, style, seed, len(feats) * cfg.stride, seed=SHARED, skip_timesteps=skip, seed_last=last,
                                   feature_division=1, windows=windows, **kw)


def _multi(cfg, lanes, d, ins, windows, per_lane, **kw):
    """`generate_clips_streams` / `generate_clips_streams_dsgplus`; `per_lane`: the edits of every lane (None: a lane without)"""
    lists = {k: [None if e is None else e[k] for e in per_lane] for k in ("inpainting_mask", "inpainted_motion", "init_motion")}
    feats = [i[0] for i in ins]
    if _zeggs(cfg):
        return S.generate_clips_streams(lanes, d, feats, ins[0][1], seed=SHARED, skip_timesteps=SKIP, kernel_set=KSET, windows=windows,
                                        **lists, **kw)
    lasts = None if ins[0][3] is None else [i[3] for i in ins]
    return S.generate_clips_streams_dsgplus(lanes, d, feats, ins[0][1], [i[2] for i in ins], len(feats[0]) * cfg.stride, seed=SHARED,
                                            skip_timesteps=SKIP, seed_lasts=lasts, feature_division=1, kernel_set=KSET, windows=windows,
                                            **lists, **kw)


def _clean(lanes):
    return all(ln.noise_streams is None and not ln.clip_init and not ln.clip_inpainting and not ln.inpainting for ln in lanes)


# ---- 1. two lanes, every option at once ----------------------------------------------------------------------------------------------------
def check_lanes(lib, cfg, K):
    """B = 2, 2 lanes, `clip_ids`; lane 0 carries a constraint and an init motion, lane 1 has None for both.  host == library; each of the
    four clips == the clip alone; the draw counter, the lanes' per-call state and their kernel sets afterwards"""
    B, n = 2, 2
    base = model(lib, cfg, PREC, B)                    # (no set named: the call's `kernel_set` is applied and put back)
    lanes = [base, base.clone(B)]
    m1, d = model(lib, cfg, PREC, 1, KSET), diffusion(lib)
    ins = [_lane_inputs(cfg, CLIPS[i], K) for i in range(n)]
    per_lane = [_edits(cfg, B, K), None]
    sets_before = [ln.kernel_set() for ln in lanes]
    got = {}
    for windows in ("host", "library"):
        got[windows] = _multi(cfg, lanes, d, ins, windows, per_lane, clip_ids=CLIP_IDS)
        assert d._draw == K * 5, (windows, d._draw)
        assert _clean(lanes), windows
        assert [ln.kernel_set() for ln in lanes] == sets_before and all(ln.last_kernel_set() == KSET for ln in lanes), windows
    klt = not _zeggs(cfg)
    assert got["host"].shape == (n * B, n_out_of(cfg, K, klt), cfg.njoints)
    assert np.array_equal(got["host"], got["library"]), (cfg.name, float(np.max(np.abs(got["host"] - got["library"]))))
    for i in range(n):
        for b in range(B):
            ins1, ed1 = _row(ins[i], per_lane[i] or {}, b)
            # (the ZEGGS multi-lane driver takes no seed pose: window 0 starts from zeros)
            alone = _single(cfg, m1, d, ins1, "library" if (i + b) % 2 else "host", seed_pose=False, stream_id=CLIP_IDS[i][b], **ed1)
            assert m1.last_kernel_set() == KSET and d._draw == K * 5 and _clean([m1])
            assert np.array_equal(got["host"][i * B + b:i * B + b + 1], alone), (cfg.name, i, b)
    assert len({got["host"][c].tobytes() for c in range(n * B)}) == n * B
    return got["host"]


# ---- 2. one lane, every option at once ------------------------------------------------------------------------------------------------------
def check_single(lib, cfg, K, edits=True, alone=False):
    """B = 2 on one lane: `clip_ids`, a constraint, an init motion and a seed pose, host against library (`alone`: and each clip alone)"""
    B = 2
    m, d = model(lib, cfg, PREC, B, KSET), diffusion(lib)
    ins = _lane_inputs(cfg, CLIPS[0], K)
    ed = _edits(cfg, B, K) if edits else {}
    got = {}
    for windows in ("host", "library"):
        got[windows] = _single(cfg, m, d, ins, windows, clip_ids=CLIP_IDS[0], **ed)
        assert d._draw == K * 5 and _clean([m]) and m.last_kernel_set() == KSET and m.kernel_set() == KSET, windows
    assert got["host"].shape == (B, n_out_of(cfg, K, not _zeggs(cfg)), cfg.njoints)
    assert np.array_equal(got["host"], got["library"]), (cfg.name, float(np.max(np.abs(got["host"] - got["library"]))))
    assert not np.array_equal(got["host"][0], got["host"][1])
    if alone:
        m1 = model(lib, cfg, PREC, 1, KSET)
        for b in range(B):
            ins1, ed1 = _row(ins, ed, b)
            one = _single(cfg, m1, d, ins1, "host" if b else "library", stream_id=CLIP_IDS[0][b], **ed1)
            assert np.array_equal(got["host"][b:b + 1], one), (cfg.name, b)


# ---- 3. DDIM ---------------------------------------------------------------------------------------------------------------------------------
def check_ddim(lib, cfg, K=2):
    """the DDIM-50 schedule, its last four steps, an init motion: host against library"""
    B = 2
    m, d = model(lib, cfg, PREC, B, KSET), create_gaussian_diffusion("ddim50", library=lib)
    ins = _lane_inputs(cfg, CLIPS[0], K)
    init = clip_init(cfg, B, K, not _zeggs(cfg))
    skip = d.num_timesteps - 4
    host = _single(cfg, m, d, ins, "host", skip=skip, ddim=True, eta=0.5, init_motion=init)
    assert d._draw == K * 5
    lib_ = _single(cfg, m, d, ins, "library", skip=skip, ddim=True, eta=0.5, init_motion=init)
    assert d._draw == K * 5 and _clean([m]) and m.last_kernel_set() == KSET
    assert np.array_equal(host, lib_), (cfg.name, float(np.max(np.abs(host - lib_))))


# ---- 4. a caller's own sample_fn ---------------------------------------------------------------------------------------------------------
def check_sample_fn(lib, cfg=C.TINY, K=2):
    """`sample_fn=spy`: the keywords the reference's loops take, for every window; the spy forwards to `p_sample_loop`"""
    m, d = model(lib, cfg, PREC, 1, KSET), diffusion(lib)
    ins, _ = _row(_lane_inputs(cfg, CLIPS[0], K), {}, 0)
    seen = []

    def spy(model_, shape, **kw):
        seen.append((model_, tuple(shape), set(kw)))
        return d.p_sample_loop(model_, shape, **kw)

    got = _single(cfg, m, d, ins, "host", sample_fn=spy)
    assert len(seen) == K
    for model_, shape, names in seen:
        assert model_ is m and shape == (1, cfg.njoints, 1, cfg.n_poses) and names == SAMPLE_FN_KEYWORDS, names
    assert np.array_equal(got, _single(cfg, m, d, ins, "host"))


# ---- 5. the queue job builder ------------------------------------------------------------------------------------------------------------
def _queue_clips(cfg, Ks, as_torch, device):
    """the clip dicts of `generate_clip_queue_dsgplus`: clip 1 has 2-D feats ([T, A] without the leading 1) and takes the default clip id;
    the clips listed in `as_torch` carry torch tensors throughout"""
    out = []
    for i, (c, K) in enumerate(zip(clips_of(cfg, Ks), Ks)):
        clip = {"feats": [f[0] if i == 1 else f for f in c["feats"]], "style": c["style"][0] if i == 2 else c["style"], "seed_pose": c["seed"],
                "seed_last": c["seed_last"], "real_n_frames": K * cfg.stride}
        if i != 1:
            clip["clip_id"] = CLIP_IDS[0][0] if i == 0 else CLIP_IDS[1][1]
        if i in as_torch:
            import torch
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            clip.update(feats=[t(f) for f in clip["feats"]], style=t(clip["style"]), seed_pose=t(clip["seed_pose"]), seed_last=t(clip["seed_last"]))
        out.append(clip)
    return out


def check_queue_jobs(lib, cfg=C.TINY5, Ks=(2, 1, 2), B=2, device="cpu"):
    """`generate_clip_queue_dsgplus` == a session of `submit`s == a session whose clip 0 is live (one window with `submit_live`, the other
    with `append(last=True, real_n_frames=...)`).  Clip 0 is made of torch tensors.  The one-shot call takes the tensor kind of ALL its
    feats from clip 0, so it runs twice: every clip numpy, and every clip torch; the sessions take clip 0 as torch beside numpy clips."""
    m, d = model(lib, cfg, PREC, B), diffusion(lib)
    set_before = m.kernel_set()                        # (no set named: the call's `kernel_set` is applied and put back)
    kw = dict(seed=SHARED, skip_timesteps=SKIP, feature_division=1, kernel_set=KSET, B=B)
    want = S.generate_clip_queue_dsgplus(m, d, _queue_clips(cfg, Ks, (), device), **kw)
    assert d._draw == max(Ks) * 5 and m.kernel_set() == set_before and m.last_kernel_set() == KSET and _clean([m])
    assert [w.shape for w in want] == [(K * cfg.stride, cfg.njoints) for K in Ks]
    as_torch = S.generate_clip_queue_dsgplus(m, d, _queue_clips(cfg, Ks, (0, 1, 2), device), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(as_torch, want))
    clips = _queue_clips(cfg, Ks, (0,), device)
    with S.open_clip_queue_dsgplus(m, d, **kw) as q:
        tickets = [q.submit(c) for c in clips]
        assert tickets == [0, 1, 2] and q.run(0) > 0
        got = [q.result(t) for t in tickets]
    assert d._draw == max(Ks) * 5 and m.kernel_set() == set_before and m.last_kernel_set() == KSET
    for i in range(len(Ks)):
        assert got[i].dtype == np.float32 and np.array_equal(got[i], want[i]), i
    with S.open_clip_queue_dsgplus(m, d, **kw) as q:
        live = {k: v for k, v in clips[0].items() if k != "real_n_frames"}
        t0 = q.submit_live(dict(live, feats=clips[0]["feats"][:1]), 2)
        tickets = [t0] + [q.submit(c) for c in clips[1:]]
        assert tickets == [0, 1, 2] and q.run(1) == 1
        q.append(t0, clips[0]["feats"][1:], last=True, real_n_frames=Ks[0] * cfg.stride)
        assert q.run(0) > 0
        got = [q.result(t) for t in tickets]
    assert d._draw == max(Ks) * 5
    for i in range(len(Ks)):
        assert np.array_equal(got[i], want[i]), i
    assert len({w.tobytes() for w in want}) == len(Ks)
