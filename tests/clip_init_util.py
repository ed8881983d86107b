"""Inputs shared by tests/test_emu_clip_init.py and tests/test_gpu_clip_init.py: a clip-level init motion (dsg_set_clip_init, `init_motion` of
the clip drivers), the index-loop restatement of the rule `sample.window_init` / k_clip_x_in implement, and the numpy restatement of the
window stitching the "kernel alone" tests use as their yardstick."""
import numpy as np

from tests.clip_inpaint_util import n_out_of


def clip_init(cfg, B, K, keep_last_tail, seed=123):
    """init [B, n_out, J]: 0.5 * randn plus a ramp over the clip's frames that differs per clip, so that a slice taken one row off, the held
    closing row and a clip handed to the wrong batch element all show"""
    n_out = n_out_of(cfg, K, keep_last_tail)
    z = 0.5 * np.random.default_rng(seed).standard_normal((B, n_out, cfg.njoints))
    ramp = np.linspace(-0.5, 0.5, n_out)[None, :, None] * (1 + np.arange(B))[:, None, None]
    return (z + ramp).astype(np.float32)


def window_init_by_index(cfg, init, seed0, c):
    """the rule of dsg_set_clip_init as an index loop: frame f of window c is clip row df = c * keep + f - S; df < 0: y['seed'] of window 0
    (zeros without one); df >= n_out: clip row n_out - 1"""
    B, n_out, J = init.shape
    w = np.zeros((B, J, 1, cfg.n_poses), np.float32)
    for f in range(cfg.n_poses):
        df = c * cfg.stride + f - cfg.n_seed
        if df < 0:
            w[:, :, 0, f] = 0.0 if seed0 is None else seed0[:, :, 0, f]
        else:
            w[:, :, 0, f] = init[:, min(df, n_out - 1)]
    return w


def numpy_stitch(zeggs, Sd, T, K, sample_window, tail):
    """tests/test_emu_clip_inpaint.py::_numpy_stitch: the K single-window samples stitched by a numpy restatement of sample.py:269-289 /
    BEAT-TWH sample.py:150-160 (fp32, the same operations in the same order); sample_window(c, seed [B, J, 1, S]) -> [B, J, 1, T];
    `tail`: y['seed'] of window 0"""
    rows = []
    for c in range(K):
        s = np.asarray(sample_window(c, np.ascontiguousarray(tail)))[:, :, 0, :].transpose(0, 2, 1).copy()      # [B, T, J]
        if c > 0:
            last0 = tail[:, :, 0, 0]
            if zeggs:
                delta = s[:, 0, :3] - last0[:, :3]
                s[:, :, :3] = s[:, :, :3] - delta[:, None, :]
            s[:, 0] = last0 * np.float32(0.5) + s[:, 0] * np.float32(0.5)
        tail = s[:, T - Sd:].transpose(0, 2, 1)[:, :, None, :]
        rows.append(s if (c == K - 1 and not zeggs) else s[:, : T - Sd])
    return np.concatenate(rows, 1)[:, Sd:]
