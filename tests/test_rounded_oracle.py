"""CPU tests of the rounded oracle (oracle/rounded.py) and of the per-row bound built on it (tests/rowcheck.py): oracle outputs only."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from oracle.mdm import MDMOracle
from oracle.rounded import PAIRS, POINTS, RoundedOracle, bf16, bf16x2
from tests import rowcheck


def _inputs(cfg, B, seed=0):
    y = synth_window_inputs(cfg, B, window=1, seed_pose_scale=0.2)
    x = np.random.RandomState(100 + B + seed).randn(B, cfg.njoints, 1, cfg.n_poses).astype(np.float32)
    return x, (np.arange(B) * 41 + 7) % 1000, y


def test_bf16_and_pair_rounding():
    """bf16(): round to nearest even on 8 mantissa bits (ties both ways); bf16x2(): hi + lo keeps 16 bits -- an error below 2^-17 relative."""
    one = np.float32(1.0)
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 3 * 2.0 ** -8)], np.float32)
    assert np.array_equal(bf16(v), np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -6)], np.float32))
    r = np.random.RandomState(0).randn(4096).astype(np.float32)
    assert np.max(np.abs(bf16(r) - r) / np.abs(r)) <= 2.0 ** -8 and np.max(np.abs(bf16x2(r) - r) / np.abs(r)) <= 2.0 ** -16
    assert bf16(one) == one and np.array_equal(bf16(bf16(r)), bf16(r))


@pytest.mark.parametrize("name", ["tiny", "tiny4", "tiny5"])
def test_no_point_on_is_the_fp32_oracle_bit_for_bit(name):
    """RoundedOracle with no rounding point returns MDMOracle's bits, probes included: variants 3 / 4 / 5, with uncond, with mask_local of
    batch 1 (with a hole), of batch B (per-clip lengths) and None."""
    cfg = C.CONFIGS[name]
    sd = synth_state_dict(cfg, 20240)
    B = 3
    x, ts, y = _inputs(cfg, B)
    m1 = np.ones((1, cfg.n_poses), bool)
    m1[:, 3:6] = False
    mB = np.arange(cfg.n_poses)[None, :] < np.array([cfg.n_poses, cfg.window + 2, cfg.window - 3])[:, None]
    for mode in ("bf16", "bf16w2"):
        a, b = MDMOracle(sd, cfg), RoundedOracle(sd, cfg, [], mode=mode)
        for uncond, mask in ((False, y["mask_local"]), (True, y["mask_local"]), (False, m1), (False, mB), (False, None), (True, mB)):
            yy = dict(y, mask_local=mask)
            wa, wb = a(x, list(ts), yy, uncond_info=uncond), b(x, list(ts), yy, uncond_info=uncond)
            assert np.isfinite(wa).all() and np.array_equal(wa, wb), (mode, uncond)
            assert a.probes.keys() == b.probes.keys() and all(np.array_equal(a.probes[k], b.probes[k]) for k in a.probes)


@pytest.mark.parametrize("name", ["tiny", "tiny4", "tiny5"])
def test_rounded_forms_are_close_and_ordered(name):
    """The library's form with no rounding (folded pose embedding, softmax normalised after P V) is the fp32 oracle to fp32 noise; every point on
    in bf16 is percent-level away, bf16w2 an order of magnitude closer, and pairing x0a as well does not move it out of that range -- in every
    variant, conditional and unconditional, with a per-clip mask; the probes are the oracle's keys."""
    cfg = C.CONFIGS[name]
    sd = synth_state_dict(cfg, 20240)
    B = 3
    x, ts, y = _inputs(cfg, B)
    mB = np.arange(cfg.n_poses)[None, :] < np.array([cfg.n_poses, cfg.window + 2, cfg.window - 3])[:, None]
    ref = MDMOracle(sd, cfg)
    for uncond, mask in ((False, y["mask_local"]), (True, None), (False, mB)):
        yy = dict(y, mask_local=mask)
        want = ref(x, list(ts), yy, uncond_info=uncond)
        rel = lambda o: float(np.linalg.norm(o(x, list(ts), yy, uncond_info=uncond).astype(np.float64) - want) / np.linalg.norm(want))
        folded = RoundedOracle(sd, cfg, [], device_form=True)
        e0, e1 = rel(folded), rel(RoundedOracle(sd, cfg, POINTS))
        e2, e3 = rel(RoundedOracle(sd, cfg, POINTS, mode="bf16w2")), rel(RoundedOracle(sd, cfg, POINTS, mode="bf16w2", pairs=PAIRS + ("x0a",)))
        assert e0 < 2e-6 and 1e-3 < e1 < 1.2e-2 and 1e-5 < e3 <= e2 * 1.5 and e2 < e1 / 4, (uncond, e0, e1, e2, e3)
        assert folded.probes.keys() == ref.probes.keys()


@pytest.fixture(scope="module")
def zeggs4():
    cfg = C.ZEGGS
    sd = synth_state_dict(cfg, 20240)
    x, ts, y = _inputs(cfg, 4)
    want, ref = rowcheck.oracle_outputs(x, ts, y, cfg, sd, "bf16")
    for a in (want, ref):
        a.setflags(write=False)
    return cfg, sd, x, ts, y, want, ref


def test_per_row_error_of_the_rounded_oracle_is_uniform_at_zeggs_dims(zeggs4):
    """What makes a per-row bound possible: with every point on, the rows of a ZEGGS batch of 4 are all about equally far from the fp32 oracle --
    median within 6e-3 ... 9e-3, max / median < 1.6 (measured: 5.8e-3 / 7.2e-3 / 9.1e-3 min / median / max)."""
    cfg, sd, x, ts, y, want, ref = zeggs4
    own = rowcheck.row_errors(ref, want)
    assert own.shape == (4, cfg.n_poses)
    print(f"per-row error of the rounded oracle: min {own.min():.2e} median {np.median(own):.2e} max {own.max():.2e}")
    assert 6e-3 < np.median(own) < 9e-3 and own.max() / np.median(own) < 1.6


def test_assert_every_row_names_one_row_scaled_by_5_percent(zeggs4):
    """The helper on oracle outputs: the rounded oracle's own output passes (ratio <= 1 by construction); the same output with ONE row -- clip 2,
    frame 37 -- scaled by 1.05 fails, and the message names that row, its token row and its 16-row tile, and no other clip."""
    cfg, sd, x, ts, y, want, ref = zeggs4
    assert rowcheck.assert_every_row(ref, x, ts, y, cfg, sd, "bf16") <= 1.0
    bad = ref.copy()
    bad[2, :, 0, 37] *= np.float32(1.05)
    with pytest.raises(AssertionError) as ei:
        rowcheck.assert_every_row(bad, x, ts, y, cfg, sd, "bf16")
    msg = str(ei.value)
    tok = 2 * (cfg.n_poses + 1) + 37 + 1
    assert "1 of 352 rows" in msg and f"(clip 2, frame 37, token row {tok}, tile {tok // 16}," in msg and "clips [2];" in msg
    nan = ref.copy()
    nan[1, 5, 0, 0] = np.nan                    # a row that is not a number is a row beyond the bound, not a row skipped
    with pytest.raises(AssertionError, match=r"clip 1, frame 0, token row 90, tile 5, inf"):
        rowcheck.assert_every_row(nan, x, ts, y, cfg, sd, "bf16")
    with pytest.raises(AssertionError):         # a result for fewer clips is no result
        rowcheck.assert_every_row(ref[:3], x, ts, y, cfg, sd, "bf16")


def test_fp32_reference_side_of_the_row_bound(zeggs4):
    """prec = "fp32": the reference is the float64 oracle, so the bound is the fp32 numpy oracle's own per-row error (6.9e-7 median, 8.2e-7 max
    measured at batch 2); a row 1e-5 off -- half the 2e-5 a whole-tensor norm allows, on ONE row -- fails at margin 4."""
    cfg, sd, x, ts, y, want, _ = zeggs4
    w2, r64 = rowcheck.oracle_outputs(x[:2], ts[:2], {k: (v[:2] if v.shape[0] == 4 else v) for k, v in y.items()}, cfg, sd, "fp32")
    assert r64.dtype == np.float64 and w2.dtype == np.float32
    own = rowcheck.row_errors(r64, w2)
    print(f"per-row error of the fp32 oracle against float64: median {np.median(own):.2e} max {own.max():.2e}")
    assert 2e-7 < np.median(own) < 2e-6 and own.max() < 3e-6
    bad = w2.copy()
    bad[1, :, 0, 80] *= np.float32(1.0 + 1e-5)
    with pytest.raises(AssertionError, match=r"clip 1, frame 80, token row 170, tile 10,"):
        rowcheck.assert_rows_within(bad, w2, r64, rowcheck.MARGIN["fp32"])
