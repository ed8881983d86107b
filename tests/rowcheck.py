"""TEST INFRASTRUCTURE: a parity bound for EVERY (clip, frame) row of a denoiser output, instead of one norm over a tensor.

For each row (b, t) -- the J pose features of frame t of clip b -- two relative errors against the fp32 oracle `want`:
    device error     |out - want| / |want|
    reference error  |ref - want| / |want|    ref = the oracle with the device's roundings (oracle/rounded.py: every point on, in the
                                              handle's precision mode); for fp32 handles the float64 oracle, so this is the fp32
                                              oracle's own error
and the condition   device error  <=  margin * max(reference error of that row, median reference error of the batch)   for ALL rows.

Margins.  bf16 / bf16w2: 2.  The device applies the same roundings to differently ordered sums, so its error is another draw from the
distribution the reference rows sample; that distribution is narrow (ZEGGS dims, synthetic weights: max / median 1.3 over the rows
of a batch), so 2 is outside its spread and still flags a row that is ~1.5 % off, where a norm over the tensor dilutes it by
sqrt(rows).  fp32: 4.  Both sides are fp32 evaluations that differ in summation order, fma contraction and the exp / erf
implementations (reference side: 7.5e-7 median, 1.2e-6 max per row at ZEGGS dims) -- still five times tighter than the 2e-5 over a
whole tensor asserted elsewhere, and local."""
import numpy as np

from oracle.mdm import MDMOracle
from oracle.rounded import PAIRS, POINTS, RoundedOracle

MARGIN = {"bf16": 2.0, "bf16w2": 2.0, "fp32": 4.0}
_ORACLES = {}      # (cfg name, id(sd), kind) -> (sd, oracle): the state dict is kept so that its id stays its own


def ref_kind(prec, kset=None):
    """Which reference models a handle of precision `prec` running kernel set `kset`."""
    return {"fp32": "fp64", "bf16": "bf16", "bf16w2": "bf16w2-rows" if kset == "rows" else "bf16w2"}[prec]


def oracle(cfg, sd, kind):
    """The oracle of one kind ("fp32" = want; "fp64", "bf16", "bf16w2", "bf16w2-rows" = references), built once per state dict."""
    key = (cfg.name, id(sd), kind)
    if key not in _ORACLES:
        if kind == "fp32":
            o = MDMOracle(sd, cfg)
        elif kind == "fp64":
            o = MDMOracle(sd, cfg, np.float64)
        elif kind == "bf16":
            o = RoundedOracle(sd, cfg, POINTS)
        elif kind == "bf16w2":         # LATENCY / TILE: the embedding output is one bf16 number
            o = RoundedOracle(sd, cfg, POINTS, mode="bf16w2")
        elif kind == "bf16w2-rows":    # ROWS: a hi + lo pair like the other A operands
            o = RoundedOracle(sd, cfg, POINTS, mode="bf16w2", pairs=PAIRS + ("x0a",))
        else:
            raise ValueError(kind)
        _ORACLES[key] = (sd, o)
    return _ORACLES[key][1]


def oracle_outputs(x, ts, y, cfg, sd, prec, uncond=False, kset=None):
    """(want, ref) for all B clips: the fp32 oracle and the reference whose distance to it models the device's error in `prec`."""
    ts = [int(t) for t in np.asarray(ts).reshape(-1)]
    want = oracle(cfg, sd, "fp32")(x, ts, y, uncond_info=uncond)
    ref = oracle(cfg, sd, ref_kind(prec, kset))(x, ts, y, uncond_info=uncond)
    return want, ref


def row_errors(a, want):
    """[B, T]: |a - want| / |want| over the J features of each (clip, frame)."""
    a, want = np.asarray(a, np.float64), np.asarray(want, np.float64)
    assert a.shape == want.shape and a.ndim == 4 and a.shape[2] == 1, (a.shape, want.shape)
    return np.linalg.norm(a - want, axis=(1, 2)) / np.linalg.norm(want, axis=(1, 2))


def assert_rows_within(out, want, ref, margin, what=""):
    """Every (clip, frame) row of `out` within margin x max(its reference error, the batch's median reference error); returns the
    largest ratio.  The failure message names the worst ten rows: clip, frame, token row b (T + 1) + t + 1 of the encoder's row
    buffer (row 0 of a clip is its conditioning token), that row's 16-row tile, ratio."""
    out = np.asarray(out)
    B, _, _, T = want.shape
    assert np.isfinite(want).all() and np.isfinite(ref).all(), f"{what}: the oracle's own output is not finite"
    dev, own = row_errors(out, want), row_errors(ref, want)
    bound = np.maximum(own, np.median(own))
    ratio = np.where(np.isfinite(dev), dev / bound, np.inf)
    assert ratio.shape == (B, T) and ratio.size == B * T          # no row is left out
    worst = float(ratio.max())
    if not worst <= margin:
        bad = np.argwhere(ratio > margin)
        order = np.argsort(-ratio.reshape(-1), kind="stable")[:10]
        rows = []
        for b, t in zip(*np.unravel_index(order, ratio.shape)):
            tok = int(b) * (T + 1) + int(t) + 1
            rows.append(f"(clip {b}, frame {t}, token row {tok}, tile {tok // 16}, {ratio[b, t]:.2f})")
        raise AssertionError(f"{what}: {len(bad)} of {B * T} rows beyond {margin:g} x the reference error (median {np.median(own):.2e}); "
                             f"clips {sorted(set(int(b) for b in bad[:, 0]))[:24]}; worst: " + ", ".join(rows))
    return worst


def assert_every_row(out, x, ts, y, cfg, sd, prec, uncond=False, kset=None):
    """`out` = the device's forward of (x, ts, y) in precision mode `prec` (kernel set `kset`: which operands bf16w2 pairs), all B
    clips: every row within MARGIN[prec] of the matching reference.  Returns the largest ratio."""
    want, ref = oracle_outputs(x, ts, y, cfg, sd, prec, uncond, kset)
    return assert_rows_within(out, want, ref, MARGIN[prec], f"{cfg.name} {prec} {kset or ''} batch {want.shape[0]}")


# ---- the inputs of the every-clip cases (tests/test_emu_rows_every_clip.py, tests/test_gpu_rows_every_clip.py) ----------------
MASK_FORMS = ("ones", "none", "perclip")


def perclip_mask(cfg, B):
    """bool [B, T]: clip b keeps frames [0, L_b), L_b = window + (7 b) mod (T - window) -- most cuts fall inside a window, and every window
    past the one after the cut is masked entirely (LocalAttention: a uniform softmax there) -- with a hole of three frames at T // 2."""
    T, w = cfg.n_poses, cfg.window
    L = w + (np.arange(B) * 7) % (T - w)
    m = np.arange(T)[None, :] < L[:, None]
    m[:, T // 2:T // 2 + 3] = False
    return m


def case_inputs(cfg, B, mask_form="ones"):
    """(x, ts, y) of one forward: distinct clips, a distinct timestep per clip, non-zero seed poses; mask_local all ones [1, T], None, or
    per clip [B, T]."""
    from diffusestylegesture_amd.synth import synth_window_inputs
    assert mask_form in MASK_FORMS
    y = synth_window_inputs(cfg, B, window=1, clip0=3, seed_pose_scale=0.2)
    if mask_form == "none":
        y["mask_local"] = None
    elif mask_form == "perclip":
        y["mask_local"] = perclip_mask(cfg, B)
    x = np.random.RandomState(100 + B).randn(B, cfg.njoints, 1, cfg.n_poses).astype(np.float32)
    return x, (np.arange(B) * 41 + 7) % 1000, y
