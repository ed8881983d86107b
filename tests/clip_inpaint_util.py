"""Inputs shared by tests/test_emu_clip_inpaint.py and tests/test_gpu_clip_inpaint.py: a clip-level inpainting constraint whose masks are
chosen for the hazards of the cut kernel (k_clip_inp_window), and the index-loop restatement of the rule it implements."""
import numpy as np

MASK_KINDS = ("block", "frames", "checker")


def n_out_of(cfg, K, keep_last_tail):
    return K * cfg.stride - (0 if keep_last_tail else cfg.n_seed)


def boundary_rows(cfg, n_out):
    """the clip rows that straddle every boundary the cut has (keep = T - S): 0; keep-S-1; keep-S = frame 0 of window 1 AND tail frame 0 of
    window 0, the blend frame; keep-1; keep; 2*keep-S = the next blend frame; n_out-1"""
    keep, S = cfg.stride, cfg.n_seed
    return [r for r in (0, keep - S - 1, keep - S, keep - 1, keep, 2 * keep - S, n_out - 1) if 0 <= r < n_out]


def clip_constraint(cfg, B, K, keep_last_tail, first=0, seed=77):
    """motion = 0.5 * randn [B, n_out, J]; mask uint8 [B, n_out, J], a different kind per clip (clip b: MASK_KINDS[(first + b) % 3]):
    block   -- features 3 .. J//2 on every frame (quads cut by the block's ends; the root channels stay free);
    frames  -- whole frames at `boundary_rows`;
    checker -- a checkerboard over (frame, feature) whose set bytes are 2 and 255, not 1.
    Every kind leaves at least half of the elements free.  Returns (mask, motion, kinds)."""
    J = cfg.njoints
    n_out = n_out_of(cfg, K, keep_last_tail)
    motion = (0.5 * np.random.default_rng(seed).standard_normal((B, n_out, J))).astype(np.float32)
    mask = np.zeros((B, n_out, J), np.uint8)
    kinds = [MASK_KINDS[(first + b) % 3] for b in range(B)]
    ff, jj = np.indices((n_out, J))
    for b, kind in enumerate(kinds):
        if kind == "block":
            mask[b, :, 3:J // 2] = 1
        elif kind == "frames":
            mask[b, boundary_rows(cfg, n_out)] = 1
        else:
            mask[b] = np.where((ff + jj) % 2 == 1, np.where((ff + jj) % 4 == 1, 2, 255), 0)
        assert 0 < np.count_nonzero(mask[b]) <= mask[b].size // 2, kind
    return mask, motion, kinds


def window_constraint_by_index(cfg, mask, motion, c):
    """the rule of dsg_set_clip_inpainting as an index loop: frame f of window c is clip row df = c * keep + f - S; constrained where
    0 <= df < n_out"""
    B, n_out, J = motion.shape
    wmask, wmotion = np.zeros((B, J, 1, cfg.n_poses), bool), np.zeros((B, J, 1, cfg.n_poses), np.float32)
    for f in range(cfg.n_poses):
        df = c * cfg.stride + f - cfg.n_seed
        if 0 <= df < n_out:
            wmask[:, :, 0, f], wmotion[:, :, 0, f] = mask[:, df] != 0, motion[:, df]
    return wmask, wmotion
