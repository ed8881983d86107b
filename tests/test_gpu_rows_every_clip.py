"""GPU: EVERY (clip, frame) row of a forward, in every batched kernel set, against the per-row bound of tests/rowcheck.py.

The other GPU files compare clips {0, B // 2, B - 1} (or one clip) of a large batch with one relative L2 norm each: at batch 46 that leaves 41
clips (about 228 of the 256 row tiles) compared with nothing, and within a compared clip a row that is 10 % off sits at the bf16 tolerance.  Here
each case is ONE forward (no chain: a chain blurs where an error sits), all B clips go through the fp32 oracle and through the oracle with the
device's roundings (oracle/rounded.py), and every row must lie within 2 x (bf16, bf16w2) / 4 x (fp32) of max(that row's reference error, the
batch's median reference error).  A fault tied to a tile index, a workgroup's slot in the weight ring, an XCD deal-out or a k_clip_attn_w chunk
boundary shows as rows / tiles named in the failure message.  The batches are the smallest that reach each code path.

Measured on MI355X (worst row of each case, as a multiple of its reference error): the table in DESIGN.md s2, profiles/r07_rows_every_clip_pytest_gpu.log."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict
from tests import rowcheck

pytestmark = pytest.mark.gpu

_SD, _ORACLE_OUT = {}, {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


def _sd(cfg):
    if cfg.name not in _SD:
        _SD[cfg.name] = synth_state_dict(cfg, 20240)
    return _SD[cfg.name]


def _model(cfg, prec, kset, max_batch):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision=prec, max_batch=max_batch, device=0).set_kernel_set(kset)
    m.load_state_dict(_sd(cfg))
    return m


def _oracle_out(cfg, B, mask_form, kind, uncond=False):
    """One oracle's output for the inputs of (cfg, B, mask_form): computed once, shared by the cases that need it, read-only."""
    key = (cfg.name, B, mask_form, kind, uncond)
    if key not in _ORACLE_OUT:
        x, ts, y = rowcheck.case_inputs(cfg, B, mask_form)
        o = rowcheck.oracle(cfg, _sd(cfg), kind)(x, [int(t) for t in ts], y, uncond_info=uncond)
        o.setflags(write=False)
        _ORACLE_OUT[key] = o
    return _ORACLE_OUT[key]


def _check(cfg, prec, kset, B, mask_form="ones"):
    x, ts, y = rowcheck.case_inputs(cfg, B, mask_form)
    m = _model(cfg, prec, kset, B)
    out = np.asarray(m(x, ts, y))
    assert m.last_kernel_set() == kset
    want, ref = _oracle_out(cfg, B, mask_form, "fp32"), _oracle_out(cfg, B, mask_form, rowcheck.ref_kind(prec, kset))
    worst = rowcheck.assert_rows_within(out, want, ref, rowcheck.MARGIN[prec], f"{cfg.name} {prec} {kset} batch {B} mask {mask_form}")
    print(f"ROWCHECK {cfg.name} {prec} {kset} batch {B} mask {mask_form}: {B * cfg.n_poses} rows, worst at {worst:.2f} x its reference error")


# dims, precision, kernel set, batch -- with the default all-ones [1, T] mask
PLAIN = [
    ("zeggs", "bf16", "latency", 1), ("zeggs", "bf16", "latency", 2),                       # the two batches `auto` gives LATENCY
    ("zeggs", "bf16", "tile", 3), ("zeggs", "bf16w2", "tile", 3), ("zeggs", "fp32", "tile", 3),    # 267 token rows: ragged last tile
    ("tiny", "bf16", "rows", 23), ("tiny", "bf16", "stream", 23),                           # the latent-128 core
    ("beat", "bf16", "tile", 1), ("twh", "bf16", "tile", 1),                                # the DSG+ batch-1 form
    ("twh", "bf16", "block", 8),                                                            # k_attn_op_w + the ff split at 512
    ("twh", "bf16", "rows", 13), ("twh", "bf16", "rows", 16),                               # 13: the smallest batch `auto` gives ROWS at 512
    ("beatpp", "bf16", "rows", 9),                                                          # variant 5 through the same kernels
    ("beatv2", "bf16", "rows", 9),                                                          # pose width 1141 at latent 384
]
# ... and these in all three mask forms (rowcheck.MASK_FORMS): all ones [1, T], None, per clip [B, T]
MASKED = [
    ("zeggs", "bf16", "block", 12), ("zeggs", "fp32", "block", 12),                         # 1068 rows, ragged; clip boundaries inside tiles
    ("zeggs", "bf16", "rows", 23), ("zeggs", "bf16", "rows", 46),                           # 2047 rows ragged; 4094 rows = 256 tiles: one full round of the CUs
    ("zeggs", "bf16w2", "rows", 16), ("zeggs", "bf16w2", "rows", 23),                       # the two-register fragments
    ("zeggs", "bf16", "stream", 23), ("zeggs", "bf16", "stream", 48),                       # 4272 rows = 267 full tiles, several blocks per workgroup; k_loc's two-wave form
    ("beat", "bf16", "block", 8),
    ("beat", "bf16", "rows", 9), ("beat", "bf16", "rows", 16),                              # 9: the smallest batch `auto` gives ROWS at 384; k_clip_attn_w chunks
]
CASES = [c + ("ones",) for c in PLAIN] + [c + (mf,) for c in MASKED for mf in rowcheck.MASK_FORMS]


@pytest.mark.parametrize("name,prec,kset,B,mask_form", CASES, ids=["-".join(str(f) for f in c) for c in CASES])
def test_every_row_of_every_clip(gpu, name, prec, kset, B, mask_form):
    """One forward of batch B on the pinned kernel set (asserted to be the set that ran), distinct timesteps and seed poses per clip: all B x T rows
    within the margin of their reference error."""
    _check(C.CONFIGS[name], prec, kset, B, mask_form)


def test_smallest_rows_batches_are_what_auto_picks(gpu):
    """The ROWS batches above named "the smallest `auto` gives it" are that: 9 at latent 384, 13 at 512; LATENCY is batch 1 and 2 in bf16."""
    for name, b in (("beat", 9), ("twh", 13)):
        m = _model(C.CONFIGS[name], "bf16", "auto", 1)
        assert [m.recommend_kernel_set(k, 1) for k in (b - 1, b)] == ["block", "rows"], name
    m = _model(C.ZEGGS, "bf16", "auto", 1)
    assert [m.recommend_kernel_set(k, 1) for k in (1, 2, 3)] == ["latency", "latency", "tile"]


def test_every_row_under_fused_guidance_in_the_stream_set(gpu):
    """Classifier-free guidance fused into the forward (dsg_set_window_cond_cfg: 12 clips + their 12 unconditional twins as one batch of 24 on
    STREAM, combined in the pose-head epilogue) against want_uncond + scale (want - want_uncond) formed from the fp32 oracle's two evaluations;
    the reference error of a row is formed the same way from the rounded oracle's two evaluations."""
    cfg, B = C.ZEGGS, 12
    x, ts, y = rowcheck.case_inputs(cfg, B)
    scale = np.linspace(0.5, 2.5, B).astype(np.float32)
    m = _model(cfg, "bf16", "stream", 2 * B)
    out = np.asarray(m.forward(x, ts, y, cfg_scale=scale))
    assert m.last_kernel_set() == "stream" and out.shape == x.shape
    s = scale.reshape(-1, 1, 1, 1)
    comb = lambda kind: _oracle_out(cfg, B, "ones", kind, True) + s * (_oracle_out(cfg, B, "ones", kind) - _oracle_out(cfg, B, "ones", kind, True))
    worst = rowcheck.assert_rows_within(out, comb("fp32"), comb("bf16"), rowcheck.MARGIN["bf16"], "zeggs bf16 stream guidance 12 + 12")
    print(f"ROWCHECK zeggs bf16 stream guidance batch 12 + 12 twins: {B * cfg.n_poses} rows, worst at {worst:.2f} x its reference error")
