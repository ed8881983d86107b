"""Clip orchestration and CLI of the sampling path -- the caller contract of the reference.

Mirrors `inference()` / `main()` / the argparse block of `main/mydiffusion_zeggs/sample.py:210-420` (ZEGGS) and
`BEAT-TWH-main/mydiffusion_beat_twh/sample.py:44-192` (DSG+): window split, per-window conditioning, seed hand-off,
root-position continuity, the one-frame blend (the reference's `len(last_poses) == 1` quirk), stitching and
de-normalisation.  The denoising itself is `sample_fn(model, shape, ...)` = `DSGDiffusion.p_sample_loop`, i.e. the
HIP library.  Windows of one clip are serially dependent (window c is seeded by window c-1), clips are independent.
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import functools
import math
import os

import numpy as np

from . import lib as L
from .diffusion import _inner_lanes

style2onehot = {
    'Happy': [1, 0, 0, 0, 0, 0], 'Sad': [0, 1, 0, 0, 0, 0], 'Neutral': [0, 0, 1, 0, 0, 0],
    'Old': [0, 0, 0, 1, 0, 0], 'Angry': [0, 0, 0, 0, 1, 0], 'Relaxed': [0, 0, 0, 0, 0, 1],
}


def _xp(use_torch):
    if use_torch:
        import torch
        return torch
    return None


def _zeggs_window_y(cfg, feat, sty, prev, seed_pose, use_torch, mask):
    """model_kwargs['y'] of one ZEGGS window (sample.py:227-251): seed poses = zeros / the caller's for window 0, the previous
    window's last n_seed frames (post-stitch) afterwards."""
    S, J = cfg.n_seed, cfg.njoints
    B = int(feat.shape[0])
    if prev is not None:
        seedp = prev[..., -S:].contiguous() if use_torch else np.ascontiguousarray(prev[..., -S:])
    elif seed_pose is not None:
        seedp = seed_pose
    elif use_torch:
        import torch
        seedp = torch.zeros(B, J, 1, S, device=feat.device)
    else:
        seedp = np.zeros((B, J, 1, S), np.float32)
    return {"style": sty, "seed": seedp, "audio": feat, "mask_local": mask}


def _zeggs_stitch(out, s, S, smoothing, use_torch):
    """sample.py:269-289: cut the overlap off the previous window, root-position continuity, the one-frame blend."""
    if out:
        last = out[-1][..., -S:]
        last = last.clone() if use_torch else last.copy()
        out[-1] = out[-1][..., :-S]
        if smoothing:
            delta = (s[:, 0:3, :, 0] - last[:, 0:3, :, 0])[..., None]
            s[:, 0:3] = s[:, 0:3] - delta
        # `for j in range(len(last_poses))` with len() == batch dim of a [1, J, 1, S] tensor: only frame 0
        s[..., 0] = last[..., 0] * 0.5 + s[..., 0] * 0.5
    out.append(s)


def _zeggs_finish(out, S, use_torch):
    out[-1] = out[-1][..., :-S]
    if use_torch:
        import torch
        seq = torch.cat([o[:, :, 0, :] for o in out], dim=2).permute(0, 2, 1)      # [B, K*stride, J]
        seq = seq[:, S:].contiguous()
        if seq.is_cuda:          # device -> PINNED host memory (torch's caching host allocator recycles the block): 23 MB per 16 clips, 1.5 -> 0.9 ms
            host = torch.empty(seq.shape, dtype=seq.dtype, pin_memory=True)
            host.copy_(seq, non_blocking=True)
            torch.cuda.current_stream(seq.device).synchronize()
            seq = host.numpy()
        else:
            seq = seq.numpy()
    else:
        seq = np.concatenate([o[:, :, 0, :] for o in out], axis=2).transpose(0, 2, 1)[:, S:]
    return np.ascontiguousarray(seq, dtype=np.float32)


def _style_batch(style, B, use_torch, dev=None):
    if L.is_torch(style):        # a tensor the caller keeps on the device: no host -> device copy per call (a small pageable copy costs
        sty = style.float()      # ~1.8 ms on ROCm -- 4 % of a 50-step DDIM pass of 4 windows, tools/prof_host.py)
        if sty.ndim == 1:
            sty = sty[None].expand(B, -1)
        return sty.to(dev).contiguous() if dev is not None else sty.contiguous()
    sty = np.asarray(style, np.float32)
    if sty.ndim == 1:
        sty = np.repeat(sty[None], B, 0)
    if use_torch:
        import torch
        return torch.from_numpy(sty).to(dev)
    return sty


def _check_windows(windows, sample_fn=None):
    """`windows=`: "host" = the window loop below, one library call per window (the default); "library" = the whole clip in one
    library call (DSGDiffusion.sample_clip: hand-off and stitching on the device; bit-identical)."""
    if windows not in ("host", "library"):
        raise ValueError(f"windows must be 'host' or 'library', not {windows!r}")
    if windows == "library" and sample_fn is not None:
        raise ValueError("windows='library' runs the library's own loops: a custom sample_fn needs windows='host'")
    return windows == "library"


def _loop_fn(diffusion, ddim, eta):
    return functools.partial(diffusion.ddim_sample_loop, eta=eta) if ddim else diffusion.p_sample_loop


def _clip_ids(clip_ids, stream_id, B, name="stream_id"):
    """`clip_ids=` of the single-lane drivers: B ints, clip i draws from the Philox stream (seed, clip_ids[i]) whichever slot it rides in
    (`DSGDiffusion.p_sample_loop(clip_streams=...)`).  Returns (stream id of the call, clip_streams keywords for the loops)."""
    if clip_ids is None:
        return (0 if stream_id is None else stream_id), {}
    if stream_id is not None:
        raise ValueError(f"clip_ids and {name} exclude each other: with clip_ids every clip has its own stream")
    ids = [int(c) for c in clip_ids]
    if len(ids) != B:
        raise ValueError(f"clip_ids: {len(ids)} entries for a batch of {B}")
    return 0, {"clip_streams": ids}


def _lane_clip_ids(clip_ids, stream_ids, n, B):
    """`clip_ids=` of the multi-lane drivers: one list of B ints per lane.  Returns (stream ids of the lanes, clip_streams keyword)."""
    if clip_ids is None:
        return (list(range(n)) if stream_ids is None else list(stream_ids)), {}
    if stream_ids is not None:
        raise ValueError("clip_ids and stream_ids exclude each other: with clip_ids every clip has its own stream")
    ids = [[int(c) for c in lane] for lane in clip_ids]
    if len(ids) != n:
        raise ValueError(f"clip_ids: {len(ids)} lists for {n} lanes")
    for lane in ids:
        if len(lane) != B:
            raise ValueError(f"clip_ids: a lane's list has {len(lane)} entries for a batch of {B}")
    return [0] * n, {"clip_streams": ids}


def window_constraint(cfg, mask, motion, c, keep_last_tail):
    """Window c's y['inpainting_mask'] / y['inpainted_motion'] (both [B, J, 1, T]) cut out of a clip-level constraint `mask` / `motion`
    [B, n_out, J] given in the coordinates of the stitched clip (n_out = K * stride - S, or K * stride with `keep_last_tail`: the DSG+
    loops).  Frame f of window c is clip row df = c * stride + f - S; for 0 <= df < n_out the window's constraint at (b, j, f) is the
    clip's at (b, df, j), elsewhere -- the first S frames of window 0, the closing S frames of the last window when they are cut -- the
    frame is unconstrained.  The tail of window c thus carries the constraint of the rows window c + 1 writes.  numpy or torch, as given;
    what the library does on the device for `windows="library"` (dsg_set_clip_inpainting)."""
    S, T, J, keep = cfg.n_seed, cfg.n_poses, cfg.njoints, cfg.n_poses - cfg.n_seed
    if (mask is None) != (motion is None):
        raise ValueError("inpainting_mask and inpainted_motion go together")
    if len(motion.shape) != 3 or int(motion.shape[2]) != J or tuple(mask.shape) != tuple(motion.shape):
        raise ValueError(f"clip constraint: mask {tuple(mask.shape)} and motion {tuple(motion.shape)} must both be [B, n_out, {J}]")
    B, n_out = int(motion.shape[0]), int(motion.shape[1])
    K, rest = divmod(n_out + (0 if keep_last_tail else S), keep)
    if rest or not 0 <= c < K:
        raise ValueError(f"clip constraint: n_out = {n_out} is not a clip of whole windows, or window {c} is outside it")
    lo = c * keep - S                                      # clip row of window frame 0
    f0, f1 = max(0, -lo), min(T, n_out - lo)
    if L.is_torch(motion):
        import torch
        wmask = torch.zeros((B, J, 1, T), dtype=torch.bool, device=motion.device)
        wmotion = torch.zeros((B, J, 1, T), dtype=torch.float32, device=motion.device)
        if f1 > f0:
            wmask[:, :, 0, f0:f1] = (torch.as_tensor(mask, device=motion.device)[:, lo + f0:lo + f1] != 0).permute(0, 2, 1)
            wmotion[:, :, 0, f0:f1] = motion[:, lo + f0:lo + f1].float().permute(0, 2, 1)
        return wmask, wmotion
    wmask, wmotion = np.zeros((B, J, 1, T), bool), np.zeros((B, J, 1, T), np.float32)
    if f1 > f0:
        wmask[:, :, 0, f0:f1] = (np.asarray(mask)[:, lo + f0:lo + f1] != 0).transpose(0, 2, 1)
        wmotion[:, :, 0, f0:f1] = np.asarray(motion, np.float32)[:, lo + f0:lo + f1].transpose(0, 2, 1)
    return wmask, wmotion


def window_init(cfg, init, seed0, c, keep_last_tail):
    """Window c's `init_image` [B, J, 1, T] cut out of a clip-level init motion `init` [B, n_out, J] given in the coordinates of the stitched
    clip (n_out = K * stride - S, or K * stride with `keep_last_tail`: the DSG+ loops) -- the clip that is noised to the first timestep and
    sampled back (gaussian_diffusion.py:701-713, for every window of the loop).  Frame f of window c is clip row df = c * stride + f - S;
    for 0 <= df < n_out the window's init at (b, j, f) is the clip's at (b, df, j).  Outside the clip: df < 0 (window 0, f < S: the frames
    the seed poses stand for) takes y['seed'] of window 0, `seed0` [B, J, 1, S] at (b, j, f), zeros without one; df >= n_out (the cut tail
    of the last window) holds clip row n_out - 1.  numpy or torch, as `init` is given; what the library does on the device for
    `windows="library"` (dsg_set_clip_init)."""
    S, T, J, keep = cfg.n_seed, cfg.n_poses, cfg.njoints, cfg.n_poses - cfg.n_seed
    if len(init.shape) != 3 or int(init.shape[2]) != J:
        raise ValueError(f"clip init_motion: shape {tuple(init.shape)} must be [B, n_out, {J}]")
    B, n_out = int(init.shape[0]), int(init.shape[1])
    K, rest = divmod(n_out + (0 if keep_last_tail else S), keep)
    if rest or K < 1 or not 0 <= c < K:
        raise ValueError(f"clip init_motion: n_out = {n_out} is not a clip of whole windows, or window {c} is outside it")
    if seed0 is not None and tuple(seed0.shape) != (B, J, 1, S):
        raise ValueError(f"clip init_motion: seed0 shape {tuple(seed0.shape)} != {(B, J, 1, S)}")
    lo = c * keep - S                                      # clip row of window frame 0
    f0, f1 = max(0, -lo), min(T, n_out - lo)               # window frames [f0, f1) lie inside the clip (f1 > f0: 2 * S < T)
    if L.is_torch(init):
        import torch
        w = torch.zeros((B, J, 1, T), dtype=torch.float32, device=init.device)
        w[:, :, 0, f0:f1] = init[:, lo + f0:lo + f1].float().permute(0, 2, 1)
        if f0 > 0 and seed0 is not None:
            w[:, :, 0, :f0] = torch.as_tensor(seed0, device=init.device).float()[:, :, 0, :f0]
        if f1 < T:
            w[:, :, 0, f1:] = init[:, n_out - 1].float()[:, :, None]
        return w
    init = np.asarray(init, np.float32)
    w = np.zeros((B, J, 1, T), np.float32)
    w[:, :, 0, f0:f1] = init[:, lo + f0:lo + f1].transpose(0, 2, 1)
    if f0 > 0 and seed0 is not None:
        w[:, :, 0, :f0] = (seed0.detach().cpu().numpy() if L.is_torch(seed0) else np.asarray(seed0, np.float32))[:, :, 0, :f0]
    if f1 < T:
        w[:, :, 0, f1:] = init[:, n_out - 1][:, :, None]
    return w


def _window_init(cfg, init, seed0, c, keep_last_tail):
    """`init_image` of window c (None without a clip-level init motion)"""
    return None if init is None else window_init(cfg, init, seed0, c, keep_last_tail)


def _per_lane_init(init_motion, n):
    """the per-lane list of the multi-lane drivers: one init motion per lane, None for a lane that starts from noise"""
    if init_motion is None:
        return [None] * n
    if len(init_motion) != n:
        raise ValueError("init_motion: one entry per lane (an entry may be None)")
    return list(init_motion)


def _constrained(y, cfg, mask, motion, c, keep_last_tail):
    """`y` of window c with the clip-level constraint's slice in it (None: `y` as it is)"""
    if mask is None and motion is None:
        return y
    if mask is None or motion is None:
        raise ValueError("inpainting_mask and inpainted_motion go together")
    wmask, wmotion = window_constraint(cfg, mask, motion, c, keep_last_tail)
    return dict(y, inpainting_mask=wmask, inpainted_motion=wmotion)


def _release_window_constraint(diffusion, models):
    """after a host window loop that put a clip-level constraint's slices into y: the lanes' sticky window-level constraint
    (`DSGDenoiser.set_inpainting`) goes with the clip it belonged to"""
    for model in models:
        inner = diffusion._library_model(model)[0]
        if inner is not None and inner.inpainting:
            inner.set_inpainting(None, None, 0)


def _per_lane(masks, motions, n):
    """the per-lane lists of the multi-lane drivers: (mask, motion) per lane, (None, None) for a lane without a constraint"""
    if masks is None and motions is None:
        return [(None, None)] * n
    if masks is None or motions is None or len(masks) != n or len(motions) != n:
        raise ValueError("inpainting_mask / inpainted_motion: one entry per lane each (an entry may be None)")
    if any((mk is None) != (mo is None) for mk, mo in zip(masks, motions)):
        raise ValueError("inpainting_mask and inpainted_motion go together")
    return list(zip(masks, motions))


def _ones_mask(T, like):
    """the all-ones y['mask_local'] [1, T] of a window: a torch tensor beside `like`, or numpy, as `like` is"""
    if L.is_torch(like):
        import torch
        return torch.ones(1, T, dtype=torch.bool, device=like.device)
    return np.ones((1, T), bool)


# The two window loops of the reference trees, as the host loop below runs them.  window_y(cfg, feats, c, sty, out, seed0, seed_last,
# use_torch, mask) -> y of window c (`out`: the windows stitched so far); stitch(out, s, S, smoothing, use_torch);
# finish(out, cfg, real_n_frames, feature_division, use_torch) -> the clip; keep_last_tail: the coordinates of the clip-level edits.
_Pipeline = collections.namedtuple("_Pipeline", "window_y stitch finish keep_last_tail")
_ZEGGS = _Pipeline(
    lambda cfg, feats, c, sty, out, seed0, seed_last, use_torch, mask:
        _zeggs_window_y(cfg, feats[c], sty, out[-1] if out else None, seed0, use_torch, mask),
    _zeggs_stitch,
    lambda out, cfg, real_n_frames, feature_division, use_torch: _zeggs_finish(out, cfg.n_seed, use_torch),
    False)
_DSGPLUS = _Pipeline(
    lambda cfg, feats, c, sty, out, seed0, seed_last, use_torch, mask:
        _dsgplus_window_y(cfg, feats, c, sty, seed0 if c == 0 else out[-1][..., -cfg.n_seed:], seed_last, use_torch, mask),
    lambda out, s, S, smoothing, use_torch: _dsgplus_stitch(out, s, S, use_torch),
    lambda out, cfg, real_n_frames, feature_division, use_torch:
        _dsgplus_finish(out, cfg.n_seed, cfg.njoints, real_n_frames, feature_division, use_torch),
    True)


def _host_windows(pipe, diffusion, lanes, feats_per_lane, stys, seed0s, seed_lasts, inp, inits, step, smoothing=False, real_n_frames=None,
                  feature_division=1, sets=None):
    """THE host window loop (`windows="host"`) of the four drivers, for n >= 1 lanes: window c of every lane gets its y (`pipe.window_y`,
    the slice of the lane's clip-level constraint `inp[i]` in it) and its `init_image` (the slice of `inits[i]`), `step(ys, init_images)`
    samples the n windows -- one library call -- and returns one [B, J, 1, T] per lane, which is stitched onto the lane's clip.  Returns
    the finished clip of every lane.  `sets`: the `_lane_kernel_sets` of a multi-lane call, in force for the windows and put back BEFORE
    the clips are finished -- finishing waits for the device, putting the sets back does not and overlaps the last window."""
    cfg = lanes[0].cfg
    n, use_torch, klt = len(lanes), L.is_torch(feats_per_lane[0][0]), pipe.keep_last_tail
    mask = _ones_mask(cfg.n_poses, feats_per_lane[0][0])
    outs = [[] for _ in range(n)]
    with sets or contextlib.nullcontext():
        for c in range(len(feats_per_lane[0])):
            ys = [_constrained(pipe.window_y(cfg, feats_per_lane[i], c, stys[i], outs[i], seed0s[i], seed_lasts[i], use_torch, mask),
                               cfg, inp[i][0], inp[i][1], c, klt) for i in range(n)]
            ss = step(ys, [_window_init(cfg, inits[i], seed0s[i], c, klt) for i in range(n)])
            for i in range(n):
                pipe.stitch(outs[i], ss[i], cfg.n_seed, smoothing, use_torch)
        if any(mk is not None for mk, _ in inp):
            _release_window_constraint(diffusion, lanes)
    return [pipe.finish(o, cfg, real_n_frames, feature_division, use_torch) for o in outs]


def _lane_step(sample_fn, model, B, skip_timesteps, keyed):
    """`step` of the single-lane drivers: the reference's call of its `sample_fn` (sample.py:253-265)"""
    shape = (B, model.cfg.njoints, 1, model.cfg.n_poses)
    return lambda ys, init_images: [sample_fn(model, shape, clip_denoised=False, model_kwargs={"y": ys[0]}, skip_timesteps=skip_timesteps,
                                              init_image=init_images[0], progress=False, dump_steps=None, noise=None, const_noise=False,
                                              **keyed)]


def _lanes_step(diffusion, lanes, B, seed, stream_ids, skip_timesteps, ddim, eta, keyed):
    """`step` of the multi-lane drivers: the lanes' windows in one `p_sample_loop_multi`"""
    shape = (B, lanes[0].cfg.njoints, 1, lanes[0].cfg.n_poses)
    return lambda ys, init_images: diffusion.p_sample_loop_multi(list(lanes), shape, [{"y": y} for y in ys], seeds=[seed] * len(lanes),
                                                                 stream_ids=stream_ids, skip_timesteps=skip_timesteps, ddim=ddim, eta=eta,
                                                                 init_images=init_images, **keyed)


def generate_clip(model, diffusion, feats, style, seed=123456, smoothing=True, skip_timesteps=0, sample_fn=None,
                  stream_id=None, seed_pose=None, device=None, *, windows="host", ddim=False, eta=0.0, inpainting_mask=None,
                  inpainted_motion=None, init_motion=None, clip_ids=None):
    """ZEGGS window loop (sample.py:236-296).  feats: sequence of K per-window WavLM features, each [B, T, A_src]
    (torch cuda tensors or numpy); style: one-hot list or [B, 6] array.  Returns normalised poses
    [B, K*stride - n_seed, J] (numpy float32) -- B independent clips advance in lock step.  `ddim` / `eta`: the DDIM loop
    instead of p_sample_loop (without a `sample_fn`); `windows`: see `_check_windows`.  `inpainting_mask` / `inpainted_motion`
    [B, K*stride - n_seed, J] (both or neither): motion inpainting over the whole clip, in the coordinates of the returned clip --
    every window runs with `window_constraint(...)` as its y['inpainting_mask'] / y['inpainted_motion'] (host loop), or the library
    cuts the same on the device (`windows="library"`).  `init_motion` [B, K*stride - n_seed, J]: an existing clip to edit, in the
    coordinates of the returned clip -- every window is noised from `window_init(...)` as its `init_image` to the timestep
    `skip_timesteps` leaves and sampled back (host loop), or the library cuts and noises the same on the device (`windows="library"`).
    `stream_id` (default 0): the Philox stream of the call, shared by the B clips (slot b of it).  `clip_ids` (B ints, instead of
    `stream_id`): clip i draws from the stream (seed, clip_ids[i]) -- the same motion in any batch, slot, lane or rank."""
    use_torch = L.is_torch(feats[0])
    B = int(feats[0].shape[0])
    stream_id, keyed = _clip_ids(clip_ids, stream_id, B)
    library = _check_windows(windows, sample_fn)
    diffusion.manual_seed(seed, stream_id)          # torch.manual_seed(seed) at sample.py:212
    sty = _style_batch(style, B, use_torch, feats[0].device if use_torch else None)
    if library:
        return diffusion.sample_clip(model, list(feats), sty, seed0=seed_pose, root_shift=smoothing, keep_last_tail=False,
                                     ddim=ddim, eta=eta, skip_timesteps=skip_timesteps, inpainting_mask=inpainting_mask,
                                     inpainted_motion=inpainted_motion, init_motion=init_motion, **keyed)
    step = _lane_step(sample_fn or _loop_fn(diffusion, ddim, eta), model, B, skip_timesteps, keyed)
    return _host_windows(_ZEGGS, diffusion, [model], [feats], [sty], [seed_pose], [None], [(inpainting_mask, inpainted_motion)], [init_motion],
                         step, smoothing)[0]


def generate_clips_streams(lanes, diffusion, feats_per_lane, styles, seed=123456, smoothing=True, skip_timesteps=0,
                           stream_ids=None, ddim=False, eta=0.0, kernel_set="recommended", *, windows="host", inpainting_mask=None,
                           inpainted_motion=None, init_motion=None, clip_ids=None):
    """Several clips of one GPU advanced concurrently on sampling LANES ("one clip per stream", BASELINE config[3]): `lanes`
    are N DSGDenoiser lanes over one copy of the weights (`model.clone()`); lane i samples the B clips of
    feats_per_lane[i] (K per-window features [B, T, A_src]; B = 1: one clip per lane) on its own HSA queue and the library
    interleaves the lanes' step loops (DSGDiffusion.p_sample_loop_multi).  Same window loop / stitching as `generate_clip`;
    lane i uses the Philox stream (seed, stream_ids[i]) and is bit-identical to `generate_clip(lanes[i], ..., stream_id=
    stream_ids[i])` run alone on the same lane.  `kernel_set`: "recommended" applies the set measured fastest for this many
    lanes x this batch to every lane (sticky: `DSGDenoiser.set_kernel_set`), None leaves the lanes as they are, a name forces
    that set.  The command processor serves one queue per compute pipe: up to 4 lanes overlap, more than 4 share pipes and
    block each other (measured: 4 lanes 2.7x one lane, 8 lanes slower than one) -- put the remaining clips into the lanes'
    batches.  `inpainting_mask` / `inpainted_motion`: per-lane lists of clip-level constraints [B, K*stride - n_seed, J] as in
    `generate_clip` (an entry may be None: that lane runs unconstrained); `init_motion`: a per-lane list of clips to edit as in
    `generate_clip` (an entry may be None: that lane starts from noise).  `clip_ids` (instead of `stream_ids`): one list of B ints per
    lane, the clip in lane i, slot b draws from the stream (seed, clip_ids[i][b]) -- any arrangement of the same clips over lanes and
    batches gives the same motion per clip under one kernel set.  Returns [N * B, K*stride - n_seed, J], lane-major."""
    n = len(lanes)
    inp = _per_lane(inpainting_mask, inpainted_motion, n)
    inits = _per_lane_init(init_motion, n)
    K = len(feats_per_lane[0])
    if any(len(f) != K for f in feats_per_lane) or len(feats_per_lane) != n:
        raise ValueError("one feature list per lane, the same number of windows each")
    use_torch = L.is_torch(feats_per_lane[0][0])
    B = int(feats_per_lane[0][0].shape[0])
    stream_ids, keyed = _lane_clip_ids(clip_ids, stream_ids, n, B)
    library, sets = _check_windows(windows), _lane_kernel_sets(lanes, B, kernel_set)
    diffusion.manual_seed(seed, 0)
    dev = feats_per_lane[0][0].device if use_torch else None
    per_lane_style = (not L.is_torch(styles)) and np.asarray(styles).ndim == 2 and len(styles) == n and np.asarray(styles).shape[0] == n and B == 1
    stys = [_style_batch(styles[i] if per_lane_style else styles, B, use_torch, dev) for i in range(n)]
    if library:
        with sets:
            seqs = diffusion.sample_clip_multi(list(lanes), [list(f) for f in feats_per_lane], stys, root_shift=smoothing,
                                               keep_last_tail=False, ddim=ddim, eta=eta, skip_timesteps=skip_timesteps,
                                               seeds=[seed] * n, stream_ids=stream_ids, inpainting_masks=[p[0] for p in inp],
                                               inpainted_motions=[p[1] for p in inp], init_motions=inits, **keyed)
    else:
        step = _lanes_step(diffusion, lanes, B, seed, stream_ids, skip_timesteps, ddim, eta, keyed)
        seqs = _host_windows(_ZEGGS, diffusion, lanes, feats_per_lane, stys, [None] * n, [None] * n, inp, inits, step, smoothing, sets=sets)
    return np.concatenate(seqs, axis=0)


class _lane_kernel_sets:
    """The kernel set of a multi-lane call: "recommended" = the set measured fastest for this many lanes x this batch (it differs
    from what one lane alone would pick), a name forces that set, None leaves the lanes alone.  A set is a sticky
    property of a lane (lanes[0] is normally the caller's own model), so whatever the call changes is put back on exit -- the
    caller's later single-lane calls run the set they ran before (round-3 advisor)."""

    def __init__(self, lanes, batch, kernel_set):
        self.lanes, self.batch, self.want, self.saved = list(lanes), batch, kernel_set, None

    def __enter__(self):
        if self.want is not None:
            self.saved = [ln.kernel_set() for ln in self.lanes]
            ks = self.lanes[0].recommend_kernel_set(self.batch, len(self.lanes)) if self.want == "recommended" else self.want
            for ln in self.lanes:
                ln.set_kernel_set(ks)
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            for ln, ks in zip(self.lanes, self.saved):
                ln.set_kernel_set(ks)
        return False


def _dsgplus_window_y(cfg, feats, c, sty, seedp, seed_last, use_torch, mask):
    """model_kwargs['y'] of window c of a DSG+ clip (BEAT-TWH sample.py:98-140) for the three model names of that tree."""
    S = cfg.n_seed
    feat = feats[c]
    seedp = seedp.contiguous() if use_torch else np.ascontiguousarray(seedp)
    y = {"style": sty, "seed": seedp, "audio": feat, "mask_local": mask}
    if cfg.variant == 3:
        # name "DiffuseStyleGesture" of the BEAT-TWH tree (attention3): S frames of left context in front of the window's
        # features -- zeros for window 0, the tail of the previous window's features afterwards (sample.py:100-102, :132-134)
        if use_torch:
            import torch
            left = torch.zeros_like(feat[:, :S]) if c == 0 else feats[c - 1][:, -S:]
            y["audio"] = torch.cat((left, feat), 1).contiguous()
        else:
            left = np.zeros_like(feat[:, :S]) if c == 0 else feats[c - 1][:, -S:]
            y["audio"] = np.ascontiguousarray(np.concatenate((left, feat), 1))
    if cfg.variant == 5:
        if seed_last is None:
            raise KeyError("seed_last")
        a = feat[:, :-S]
        y["audio"] = a.contiguous() if use_torch else np.ascontiguousarray(a)
        y["seed_last"] = seed_last
    return y


def _dsgplus_stitch(out, s, S, use_torch):
    """BEAT-TWH sample.py:150-160: cut the overlap off the previous window, the one-frame blend; no root shift."""
    if out:
        last = out[-1][..., -S:]
        last = last.clone() if use_torch else last.copy()
        out[-1] = out[-1][..., :-S]
        s[..., 0] = last[..., 0] * 0.5 + s[..., 0] * 0.5
    out.append(s)


def _dsgplus_library(diffusion, lanes, feats_per_lane, sty, seed0s, seed_lasts, real_n_frames, feature_division, seed, stream_ids,
                     skip_timesteps, ddim, eta, inp=None, inits=None, keyed=None):
    """The DSG+ clips of every lane through DSGDiffusion.sample_clip_multi: the per-window features as `_dsgplus_window_y` builds them,
    then crop + feature division as `_dsgplus_finish`."""
    cfg = lanes[0].cfg
    use_torch = L.is_torch(feats_per_lane[0][0])
    audio = [[_dsgplus_window_y(cfg, f, c, sty, seed0s[i], None if seed_lasts is None else seed_lasts[i], use_torch, None)["audio"]
              for c in range(len(f))] for i, f in enumerate(feats_per_lane)]
    seqs = diffusion.sample_clip_multi(list(lanes), audio, [sty] * len(lanes), seed0s=list(seed0s), root_shift=False, keep_last_tail=True,
                                       ddim=ddim, eta=eta, skip_timesteps=skip_timesteps, seed_lasts=seed_lasts, seeds=[seed] * len(lanes),
                                       stream_ids=stream_ids, inpainting_masks=None if inp is None else [p[0] for p in inp],
                                       inpainted_motions=None if inp is None else [p[1] for p in inp], init_motions=inits, **(keyed or {}))
    return [np.ascontiguousarray(q[:, :real_n_frames, : cfg.njoints // feature_division], dtype=np.float32) for q in seqs]


def _dsgplus_finish(out, S, J, real_n_frames, feature_division, use_torch):
    if use_torch:
        import torch
        seq = torch.cat([o[:, :, 0, :] for o in out], dim=2).permute(0, 2, 1).contiguous().cpu().numpy()
    else:
        seq = np.concatenate([o[:, :, 0, :] for o in out], axis=2).transpose(0, 2, 1)
    seq = seq[:, S:][:, :real_n_frames]
    # "v0" data: the model features are poses + velocities + accelerations, only the poses are kept (motion_feature_division = 3,
    # BEAT-TWH sample.py:173-180); "v2": the whole vector (division 1)
    return np.ascontiguousarray(seq[:, :, : J // feature_division], dtype=np.float32)


def generate_clips_streams_dsgplus(lanes, diffusion, feats_per_lane, styles, seed0s, real_n_frames, seed=123456, skip_timesteps=0,
                                   stream_ids=None, seed_lasts=None, feature_division=3, ddim=False, eta=0.0,
                                   kernel_set="recommended", *, windows="host", inpainting_mask=None, inpainted_motion=None,
                                   init_motion=None, clip_ids=None):
    """`generate_clips_streams` for the DSG+ window loop (BEAT-TWH sample.py:98-192; all three model names of that tree): lane i
    samples the B clips of feats_per_lane[i] (K per-window features), seeded by seed0s[i] [B, J, 1, S] (and seed_lasts[i] for
    DiffuseStyleGesture++), on its own HSA queue; the lanes' step loops are interleaved by the library.  Lane i is bit-identical
    to `generate_clip_dsgplus(lanes[i], ..., stream_id=stream_ids[i])` run alone on the same lane under the same kernel set.
    `inpainting_mask` / `inpainted_motion`: per-lane lists of clip-level constraints [B, K*stride, J] as in `generate_clip_dsgplus`
    (an entry may be None); `init_motion`: a per-lane list of clips [B, K*stride, J] to edit (an entry may be None); `clip_ids`: one list
    of B ints per lane instead of `stream_ids`, every clip its own stream as in `generate_clips_streams`.  Returns
    [N * B, real_n_frames, J // feature_division], lane-major."""
    n = len(lanes)
    inp = _per_lane(inpainting_mask, inpainted_motion, n)
    inits = _per_lane_init(init_motion, n)
    K = len(feats_per_lane[0])
    if any(len(f) != K for f in feats_per_lane) or len(feats_per_lane) != n or len(seed0s) != n:
        raise ValueError("one feature list and one seed clip per lane, the same number of windows each")
    use_torch = L.is_torch(feats_per_lane[0][0])
    B = int(feats_per_lane[0][0].shape[0])
    stream_ids, keyed = _lane_clip_ids(clip_ids, stream_ids, n, B)
    library, sets = _check_windows(windows), _lane_kernel_sets(lanes, B, kernel_set)
    diffusion.manual_seed(seed, 0)
    sty = _style_batch(styles, B, use_torch, feats_per_lane[0][0].device if use_torch else None)
    if library:
        with sets:
            seqs = _dsgplus_library(diffusion, lanes, feats_per_lane, sty, seed0s, seed_lasts, real_n_frames, feature_division,
                                    seed, stream_ids, skip_timesteps, ddim, eta, inp, inits, keyed)
    else:
        step = _lanes_step(diffusion, lanes, B, seed, stream_ids, skip_timesteps, ddim, eta, keyed)
        seqs = _host_windows(_DSGPLUS, diffusion, lanes, feats_per_lane, [sty] * n, seed0s, [None] * n if seed_lasts is None else seed_lasts,
                             inp, inits, step, real_n_frames=real_n_frames, feature_division=feature_division, sets=sets)
    return np.concatenate(seqs, axis=0)


def generate_clip_dsgplus(model, diffusion, feats, style, seed0, real_n_frames, seed=123456, skip_timesteps=0,
                          sample_fn=None, stream_id=None, seed_last=None, feature_division=3, *, windows="host", ddim=False, eta=0.0,
                          inpainting_mask=None, inpainted_motion=None, init_motion=None, clip_ids=None):
    """DSG+ window loop (BEAT-TWH sample.py:98-192), attention4: zero-padded tail, no left audio context, GT seed for
    window 0, no root shift, last window kept whole, first S frames dropped, crop, keep the first J/3 features.
    `model.cfg.variant == 3` is that tree's "DiffuseStyleGesture" (attention3 at BEAT dims): S frames of left audio context.
    DiffuseStyleGesture++ (attention5, model.cfg.variant == 5): `feats` are still the stride-long windows; the last S
    feature frames of every window are dropped (sample.py:104, :138) and `seed_last` [B, J, 1, S] -- the same snippet
    for every window (sample.py:85-93) -- is passed as y['seed_last'].  `inpainting_mask` / `inpainted_motion` [B, K*stride, J]
    (both or neither): motion inpainting over the whole clip as in `generate_clip`, in the coordinates of the stitched clip: the full J
    features, before the crop to `real_n_frames` and the feature division.  `init_motion` [B, K*stride, J]: an existing clip to edit as in
    `generate_clip`, in the same coordinates (the full J features, K*stride frames).  `stream_id` (default 0) / `clip_ids` (B ints: every
    clip its own Philox stream (seed, clip_ids[i])) as in `generate_clip`."""
    use_torch = L.is_torch(feats[0])
    B = int(feats[0].shape[0])
    stream_id, keyed = _clip_ids(clip_ids, stream_id, B)
    library = _check_windows(windows, sample_fn)
    diffusion.manual_seed(seed, stream_id)
    sty = _style_batch(style, B, use_torch, feats[0].device if use_torch else None)
    if library:
        return _dsgplus_library(diffusion, [model], [feats], sty, [seed0], None if seed_last is None else [seed_last], real_n_frames,
                                feature_division, seed, [stream_id], skip_timesteps, ddim, eta,
                                _per_lane(None if inpainting_mask is None else [inpainting_mask],
                                          None if inpainted_motion is None else [inpainted_motion], 1),
                                None if init_motion is None else [init_motion],
                                {"clip_streams": [keyed["clip_streams"]]} if keyed else None)[0]
    step = _lane_step(sample_fn or _loop_fn(diffusion, ddim, eta), model, B, skip_timesteps, keyed)
    return _host_windows(_DSGPLUS, diffusion, [model], [feats], [sty], [seed0], [seed_last], [(inpainting_mask, inpainted_motion)], [init_motion],
                         step, real_n_frames=real_n_frames, feature_division=feature_division)[0]


def _queue_lanes(lanes, clips, B):
    """(the lanes' DSGDenoisers, guided, B) of a clip-queue call: guidance is on when any clip carries a scale; B defaults to
    min(max_batch, ceil(N / lanes)) -- max_batch halved with guidance, the twins ride in the same batch."""
    inners, _ = _inner_lanes(lanes, "sample_clip_queue")
    guided = any(c.get("scale") is not None for c in clips)
    if B is None:
        room = min(m.max_batch for m in inners) // (2 if guided else 1)
        B = max(1, min(room, -(-len(clips) // len(inners))))
    return inners, guided, int(B)


def _queue_job(cfg, clip, i, dsgplus, live=False):
    """One clip dict of the queue drivers as the job dict `DSGDiffusion.sample_clip_queue` / `ClipQueue.submit[_live]` take: the style
    flat, "seed_pose" as "seed0", "clip_id" (default `i`: the clip's index or ticket) as "stream", the clip's edits and its own
    "skip_timesteps" passed through; DSG+: the per-window features as `_dsgplus_window_y` builds them.  `live`: a live clip -- no edits,
    and "feats" are taken as they are (`_ClipQueueSession._window_audio` has built them)."""
    c = clip
    job = {"feats": c["feats"], "style": c["style"] if L.is_torch(c["style"]) else np.asarray(c["style"], np.float32).reshape(-1),
           "seed0": c.get("seed_pose"), "scale": c.get("scale"), "stream": int(c.get("clip_id", i))}
    job.update({k: c[k] for k in (("skip_timesteps",) if live else ("inpainting_mask", "inpainted_motion", "init_motion", "skip_timesteps"))
                if c.get(k) is not None})
    if dsgplus:
        job["seed0"], job["seed_last"] = c["seed_pose"], c.get("seed_last")
        if not live:
            feats = [f if f.ndim == 3 else f[None] for f in c["feats"]]
            job["feats"] = [_dsgplus_window_y(cfg, feats, w, None, c["seed_pose"], c.get("seed_last"), L.is_torch(feats[0]), None)["audio"]
                            for w in range(len(feats))]
    return job


def generate_clip_queue(lanes, diffusion, clips, seed=123456, smoothing=True, skip_timesteps=0, ddim=False, eta=0.0,
                        kernel_set="recommended", *, B=None):
    """ZEGGS clips of DIFFERENT lengths through `DSGDiffusion.sample_clip_queue`: the clips share the `lanes` x `B` slots and a slot takes
    the next clip when its clip ends, so no round is spent on padding (`lib.clip_queue_plan`).  `lanes`: a DSGDenoiser or a list of lanes
    (`model.clone()`).  `clips`: one dict per clip -- "feats": its K_i per-window WavLM features, each [T, A_src] or [1, T, A_src];
    "style": one-hot list or [6] array; optional "seed_pose" [1, J, 1, S] (default zeros), "scale" (classifier-free guidance for the whole
    call as soon as one clip has it; the others run at scale 1), "clip_id" (default: the clip's index), and the clip's own edits
    "inpainting_mask" / "inpainted_motion" / "init_motion", each [K_i*stride - n_seed, J] (or [1, ...]) as `generate_clip` takes them for
    that clip, and "skip_timesteps", the clip's own (default: the keyword): fresh generations and edits of any depth share one queue.
    All clips share `seed`; clip i draws
    from the Philox stream (seed, clip_id) and is bit for bit `generate_clip(lane of batch 1, ..., windows="library", stream_id=clip_id)`
    with the clip's edits under the same kernel set.  `kernel_set` as in `generate_clips_streams`.  Returns a list of [K_i*stride - n_seed, J] arrays in the
    order given."""
    clips = list(clips)
    inners, guided, B = _queue_lanes(lanes, clips, B)
    jobs = [_queue_job(inners[0].cfg, c, i, False) for i, c in enumerate(clips)]
    with _lane_kernel_sets(inners, B, kernel_set):
        diffusion.manual_seed(seed, 0)
        return diffusion.sample_clip_queue(inners, jobs, B, root_shift=smoothing, keep_last_tail=False, ddim=ddim, eta=eta,
                                           skip_timesteps=skip_timesteps, guided=guided)


def generate_clip_queue_dsgplus(lanes, diffusion, clips, seed=123456, skip_timesteps=0, feature_division=3, ddim=False, eta=0.0,
                                kernel_set="recommended", *, B=None):
    """`generate_clip_queue` for the DSG+ window loop (all three model names of that tree): every clip dict carries "feats" (K_i
    stride-long windows, each [1, T, A_src]), "style", "seed_pose" [1, J, 1, S] (the ground-truth seed of window 0), "real_n_frames", and
    for DiffuseStyleGesture++ "seed_last" [1, J, 1, S]; optional "scale", "clip_id", and the clip's own edits "inpainting_mask" /
    "inpainted_motion" / "init_motion" in the [K_i*stride, J] coordinates `generate_clip_dsgplus` documents (all J features, before the
    crop and the feature division) and its own "skip_timesteps" (default: the keyword).  The per-window features are built as
    `_dsgplus_window_y` builds them; every clip is finished as `_dsgplus_finish` finishes it -- cropped to ITS real_n_frames, the first
    J // feature_division features kept.  Clip i is bit for bit `generate_clip_dsgplus(lane of batch 1, ..., windows="library",
    stream_id=clip_id)`.  Returns a list of [real_n_frames_i, J // feature_division] arrays in the order given."""
    clips = list(clips)
    inners, guided, B = _queue_lanes(lanes, clips, B)
    cfg = inners[0].cfg
    jobs = [_queue_job(cfg, c, i, True) for i, c in enumerate(clips)]
    with _lane_kernel_sets(inners, B, kernel_set):
        diffusion.manual_seed(seed, 0)
        seqs = diffusion.sample_clip_queue(inners, jobs, B, root_shift=False, keep_last_tail=True, ddim=ddim, eta=eta,
                                           skip_timesteps=skip_timesteps, guided=guided)
    return [np.ascontiguousarray(q[: int(c["real_n_frames"]), : cfg.njoints // feature_division], dtype=np.float32) for q, c in zip(seqs, clips)]


class _ClipQueueSession:
    """What `open_clip_queue` / `open_clip_queue_dsgplus` return: `DSGDiffusion.open_clip_queue` behind the clip dicts of
    `generate_clip_queue[_dsgplus]`.  The lanes keep the session's kernel set from open to close (a set cannot change while a session owns
    the lane); close puts back what they ran before, as `_lane_kernel_sets` does."""

    def __init__(self, lanes, diffusion, dsgplus, seed, skip_timesteps, ddim, eta, kernel_set, B, guided, root_shift, feature_division):
        inners, wrapped = _inner_lanes(lanes, "open_clip_queue")
        guided = bool(guided) or any(wrapped)
        if B is None:
            B = max(1, min(m.max_batch for m in inners) // (2 if guided else 1))
        self.cfg, self.dsgplus, self.feature_division, self._real, self._n = inners[0].cfg, dsgplus, feature_division, {}, 0
        self._live = {}                                  # ticket of a live clip -> [seed_pose, seed_last, the last window given] (DSG+)
        self._sets = _lane_kernel_sets(inners, int(B), kernel_set)
        self._sets.__enter__()
        try:
            diffusion.manual_seed(seed, 0)
            self.queue = diffusion.open_clip_queue(inners, int(B), root_shift=root_shift, keep_last_tail=dsgplus, ddim=ddim, eta=eta,
                                                   skip_timesteps=skip_timesteps, guided=guided)
        except Exception:
            self._sets.__exit__(None, None, None)
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def submit(self, clip, priority=0) -> int:
        """One clip dict of `generate_clip_queue` (`generate_clip_queue_dsgplus` for a DSG+ session); "clip_id" defaults to the ticket.
        `priority` (or a "priority" key of the dict) as `ClipQueue.submit`: higher runs first, default 0."""
        t = self.queue.submit(_queue_job(self.cfg, clip, self._n, self.dsgplus), priority=clip.get("priority", priority))
        self._n += 1
        if self.dsgplus:
            self._real[t] = int(clip["real_n_frames"])
        return t

    def _window_audio(self, ticket, feats):
        """the per-window features of a live clip as the library takes them; DSG+: as `_dsgplus_window_y` builds them (the attention3 model
        puts the tail of the window before in front, so the last window given is kept per ticket)"""
        feats = list(feats) if isinstance(feats, (list, tuple)) else [feats]
        if not self.dsgplus or not feats:
            return feats
        use_torch = L.is_torch(feats[0])
        seed_pose, seed_last, prev = self._live[ticket]
        feats = [f if f.ndim == 3 else f[None] for f in feats]
        chain = ([prev] if prev is not None else []) + feats
        at = len(chain) - len(feats)
        # (index 0 of the chain -- the zero left context -- is a window of this call only when it is the clip's first)
        audio = [_dsgplus_window_y(self.cfg, chain, at + w, None, seed_pose, seed_last, use_torch, None)["audio"] for w in range(len(feats))]
        self._live[ticket][2] = feats[-1]
        return audio

    def submit_live(self, clip, capacity, priority=0) -> int:
        """A live clip (`ClipQueue.submit_live`): the clip dict of `submit` without edits and without "real_n_frames"; "feats" are the
        windows known now and may be empty; `capacity`: the most windows it may ever get.  Feed it with `append`, end it with `finish`.
        `priority` as for `submit`."""
        ticket = self._n                                 # (tickets count submissions)
        self._live[ticket] = [clip["seed_pose"], clip.get("seed_last"), None] if self.dsgplus else None
        job = _queue_job(self.cfg, dict(clip, feats=self._window_audio(ticket, clip.get("feats") or [])), ticket, self.dsgplus, live=True)
        t = self.queue.submit_live(job, capacity, priority=clip.get("priority", priority))
        assert t == ticket
        self._n += 1
        return t

    def append(self, ticket, feats, style=None, scale=None, last=False, real_n_frames=None):
        """Further windows for a live clip (`ClipQueue.append`); `last=True` finishes it (DSG+: `real_n_frames` as for `finish`)."""
        if style is not None and not L.is_torch(style):
            style = np.asarray(style, np.float32).reshape(-1)
        if last and self.dsgplus and real_n_frames is not None:
            self._real[int(ticket)] = int(real_n_frames)
        self.queue.append(ticket, self._window_audio(int(ticket), feats), style=style, scale=scale, last=last)

    def finish(self, ticket, real_n_frames=None):
        """No more windows for a live clip.  DSG+: `result` / `rows` crop to `real_n_frames` as `submit` does (None: no crop in time)."""
        if self.dsgplus and real_n_frames is not None:
            self._real[int(ticket)] = int(real_n_frames)
        self.queue.finish(ticket)

    def _crop(self, ticket, q):
        if not self.dsgplus:
            return q
        return np.ascontiguousarray(q[: self._real.get(int(ticket)), : self.cfg.njoints // self.feature_division], dtype=np.float32)

    def set_priority(self, ticket, priority):
        self.queue.set_priority(ticket, priority)

    def park(self, ticket):
        """`ClipQueue.park`: the clip waits -- a running one leaves its slot at the next round -- until `resume`"""
        self.queue.park(ticket)

    def resume(self, ticket):
        self.queue.resume(ticket)

    def run(self, max_rounds=1) -> int:
        return self.queue.run(max_rounds)

    def job(self, ticket) -> dict:
        return self.queue.job(ticket)

    def rows(self, ticket):
        """the rows that are final so far (DSG+: cropped to the clip's real_n_frames and feature division, as `result`)"""
        return self._crop(ticket, self.queue.rows(ticket))

    def result(self, ticket):
        """the finished clip, as `generate_clip_queue[_dsgplus]` returns it; raises unless it is done"""
        return self._crop(ticket, self.queue.result(ticket))

    def cancel(self, ticket):
        self.queue.cancel(ticket)

    def close(self):
        if self._sets is None:
            return
        sets, self._sets = self._sets, None
        try:
            self.queue.close()
        finally:
            sets.__exit__(None, None, None)


def open_clip_queue(lanes, diffusion, seed=123456, smoothing=True, skip_timesteps=0, ddim=False, eta=0.0, kernel_set="recommended", *, B=None,
                    guided=False):
    """`generate_clip_queue` as a session: submit ZEGGS clip dicts while it runs, collect rows per window (`DSGDiffusion.open_clip_queue`).
    Returns a context manager with submit / run / job / rows / result / cancel / close, submit_live / append / finish for a clip whose
    windows arrive while it runs, and set_priority / park / resume (`submit(clip, priority=)`: higher runs first and pre-empts).  `guided` is fixed at open (a lane wrapped in
    ClassifierFreeSampleModel turns it on); B defaults to the lanes' max_batch (halved with guidance).  Clip i is bit for bit
    `generate_clip(lane of batch 1, ..., windows="library", stream_id=clip_id)` whenever it was submitted."""
    return _ClipQueueSession(lanes, diffusion, False, seed, skip_timesteps, ddim, eta, kernel_set, B, guided, smoothing, 1)


def open_clip_queue_dsgplus(lanes, diffusion, seed=123456, skip_timesteps=0, feature_division=3, ddim=False, eta=0.0, kernel_set="recommended", *,
                            B=None, guided=False):
    """`generate_clip_queue_dsgplus` as a session: the windows are built as `_dsgplus_window_y` builds them, `result` / `rows` crop as
    `_dsgplus_finish` does."""
    return _ClipQueueSession(lanes, diffusion, True, seed, skip_timesteps, ddim, eta, kernel_set, B, guided, False, feature_division)


def window_audio(audio, n_frames, n_poses=88, n_seed=8, sr=16000, fps=20):
    """Audio slices per window with the n_seed-frame left context (sample.py:214-249): zeros for window 0, the
    previous chunk's tail otherwise.  Returns (list of float32 arrays of (n_poses * sr/fps) samples, n_frames)."""
    if n_frames == 0:
        n_frames = audio.shape[0] * fps // sr
    stride = n_poses - n_seed
    if n_frames < stride:
        k = 1
    else:
        k = math.floor(n_frames / stride)
        n_frames = k * stride
    spf = sr // fps
    audio = np.asarray(audio[: n_frames * spf], np.float32)
    chunks = audio.reshape(k, stride * spf)
    outs = []
    for c in range(k):
        left = np.zeros(n_seed * spf, np.float32) if c == 0 else chunks[c - 1][-n_seed * spf:]
        outs.append(np.concatenate([left, chunks[c]]))
    return outs, n_frames


def load_wav_16k(path):
    """Mono float32 waveform at 16 kHz in [-1, 1] (what `librosa.load(path, sr=16000)` returns, sample.py:346; librosa is
    not a dependency here: scipy reads the file and resamples polyphase when the file's rate differs)."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    sr, x = wavfile.read(path)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    else:
        x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    if sr != 16000:
        g = math.gcd(int(sr), 16000)
        x = resample_poly(x, 16000 // g, int(sr) // g).astype(np.float32)
    return x


def denormalise(poses, mean, std):
    """sample.py:320-326: std clipped at 0.01."""
    return np.multiply(poses, np.clip(std, a_min=0.01, a_max=None)) + mean


def inference(args, wavlm_model, audio, sample_fn, model, n_frames=0, smoothing=False, SG_filter=False,
              minibatch=False, skip_timesteps=0, n_seed=8, style=None, seed=123456, *, diffusion=None,
              wav2wavlm=None, mean=None, std=None, pose_writer=None, save_path=None):
    """Same positional signature as the reference `inference()` (sample.py:210).  `wav2wavlm(wavlm_model, wav)` must
    return the [1, n_poses, 1024] WavLM features of one window (the WavLM encoder stays on PyTorch-ROCm, outside this
    path); `pose_writer(out_poses, path, length, smoothing)` is the BVH writer.  Returns de-normalised poses."""
    if not minibatch:
        raise NotImplementedError("only the minibatch (windowed) path of inference() is on the sampling path")
    if diffusion is None:
        diffusion = sample_fn.__self__
    wins, n_frames = window_audio(audio, n_frames, args.n_poses, n_seed)
    feats = [wav2wavlm(wavlm_model, w) for w in wins]
    poses = generate_clip(model, diffusion, feats, style, seed=seed, smoothing=smoothing,
                          skip_timesteps=skip_timesteps, sample_fn=sample_fn)[0]
    out_poses = denormalise(poses, mean, std) if mean is not None else poses
    if pose_writer is not None and save_path is not None:
        pose_writer(out_poses, save_path, length=n_frames - n_seed, smoothing=SG_filter)
    return out_poses


def build_parser():
    p = argparse.ArgumentParser(description='DiffuseStyleGesture')          # flags of sample.py:400-407
    p.add_argument('--config', default='./configs/DiffuseStyleGesture.yml')
    p.add_argument('--gpu', type=str, default='0')
    p.add_argument('--no_cuda', type=list, default=['2'])
    p.add_argument('--model_path', type=str, default='./model000450000.pt')
    p.add_argument('--audiowavlm_path', type=str, default='')
    p.add_argument('--max_len', type=int, default=0)
    # framework additions
    p.add_argument('--precision', default='bf16', choices=['bf16', 'bf16w2', 'fp32'],
                   help='bf16 (default); bf16w2 = bf16 activations, weights as hi + lo bf16 (3x closer to fp32); fp32 = the reference arithmetic')
    p.add_argument('--features_npy', default='', help='pre-extracted WavLM features [K, n_poses, 1024] (the per-clip cache)')
    p.add_argument('--wavlm_path', default='./WavLM/WavLM-Large.pt', help='WavLM checkpoint (sample.py:33)')
    p.add_argument('--save_dir', default='sample_dir')
    p.add_argument('--timestep_respacing', default='')
    p.add_argument('--windows', default='host', choices=['host', 'library'],
                   help='host = one library call per window, stitched on the host (default); library = the whole clip in one library call')
    p.add_argument('--skip_timesteps', type=int, default=0, help='start the denoising this many timesteps below the last one')
    p.add_argument('--init_npy', default='',
                   help='edit an existing clip: normalised poses [n_out, J] or [1, n_out, J] (n_out = K * stride - n_seed, what --save_dir/*_poses.npy '
                        'holds) are noised to the timestep --skip_timesteps leaves and sampled back under this run\'s style and audio')
    return p


def load_init_npy(path, n_out, J, B=1):
    """--init_npy: normalised poses [n_out, J] (one clip, repeated for every clip of the batch) or [B, n_out, J]"""
    a = np.asarray(np.load(path), np.float32)
    if a.ndim == 2:
        a = np.repeat(a[None], B, 0)
    if a.shape != (B, n_out, J):
        raise SystemExit(f"--init_npy: shape {a.shape} is not [{n_out}, {J}] or [{B}, {n_out}, {J}]")
    return np.ascontiguousarray(a)


def main(argv=None):
    import yaml
    import torch
    from .config import ZEGGS
    from .diffusion import create_gaussian_diffusion
    from .model import DSGDenoiser
    args = build_parser().parse_args(argv)
    cfg_yaml = {}
    if os.path.exists(args.config):
        with open(args.config) as f:
            cfg_yaml = yaml.safe_load(f) or {}
    n_poses = int(cfg_yaml.get("n_poses", ZEGGS.n_poses))
    assert n_poses == ZEGGS.n_poses
    dev = int(args.gpu)
    torch.cuda.set_device(dev)
    model = DSGDenoiser(ZEGGS, precision=args.precision, max_batch=1, device=dev)
    state_dict = torch.load(args.model_path, map_location='cpu')
    model.load_state_dict(state_dict)
    diffusion = create_gaussian_diffusion(args.timestep_respacing)
    name = os.path.basename(args.audiowavlm_path or args.features_npy)
    style = style2onehot[name.split('_')[1]]                              # sample.py:378
    os.makedirs(args.save_dir, exist_ok=True)
    if args.features_npy:
        feats = np.load(args.features_npy).astype(np.float32)
    else:
        # WavLM stage (PyTorch-ROCm, outside the HIP path): all windows of the clip in ONE batched forward, cached per clip
        from .wavlm import wavlm_init
        wav = load_wav_16k(args.audiowavlm_path)                          # librosa.load(path, sr=16000), sample.py:346
        wins, _ = window_audio(wav, args.max_len, n_poses, ZEGGS.n_seed)
        wavlm = wavlm_init(args.wavlm_path, device=f"cuda:{dev}")
        feats = wavlm.clip_features(wins, n_poses).cpu().numpy()
        np.save(os.path.join(args.save_dir, os.path.splitext(name)[0] + "_wavlm.npy"), feats)
        del wavlm
    if args.max_len:
        feats = feats[: max(1, args.max_len // (n_poses - ZEGGS.n_seed))]
    feats_t = [torch.from_numpy(f[None]).cuda(dev) for f in feats]
    init = load_init_npy(args.init_npy, len(feats_t) * ZEGGS.stride - ZEGGS.n_seed, ZEGGS.njoints) if args.init_npy else None
    poses = generate_clip(model, diffusion, feats_t, style, seed=123456, smoothing=True, skip_timesteps=args.skip_timesteps,
                          windows=args.windows, init_motion=init)[0]
    stem = os.path.join(args.save_dir, os.path.splitext(name)[0])
    np.save(stem + "_poses.npy", poses)
    # de-normalise (sample.py:320-326) and write the .bvh (process_zeggs_bvh.py:219) like the reference's main()
    from .bvh import pose2bvh
    ms = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "zeggs_mean_std.npz"))
    out_poses = denormalise(poses, ms["mean"], ms["std"])
    pose2bvh(out_poses, stem + ".bvh", length=out_poses.shape[0], smoothing=True)      # C++ writer (csrc/dsg_bvh.cpp)
    print(stem + ".bvh", out_poses.shape)
    return stem + ".bvh"


if __name__ == '__main__':
    main()
