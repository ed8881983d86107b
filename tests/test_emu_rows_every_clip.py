"""CPU: every (clip, frame) row of a forward under the SIMT emulator against the per-row bound of tests/rowcheck.py -- the tiny dims of all
three variants, in bf16 and bf16w2, in every kernel set that accepts them.  This proves the helper and the rounded oracle (oracle/rounded.py)
against the product sources without a GPU; tests/test_gpu_rows_every_clip.py has the real dims on the device."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.model import DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict
from tests import rowcheck

# what each (dims, precision) accepts (the others are DSG_E_NOT_IMPLEMENTED: ROWS / STREAM need latent_dim 128 / 256 ... and bf16; bf16w2 has no BLOCK)
SETS = {("tiny", "bf16"): ("latency", "tile", "block", "rows", "stream"), ("tiny", "bf16w2"): ("latency", "tile", "rows"),
        ("tiny4", "bf16"): ("latency", "tile", "block"), ("tiny4", "bf16w2"): ("latency", "tile"),
        ("tiny5", "bf16"): ("latency", "tile", "block"), ("tiny5", "bf16w2"): ("latency", "tile")}
_SD, _WANT = {}, {}


def _sd(cfg):
    if cfg.name not in _SD:
        _SD[cfg.name] = synth_state_dict(cfg, 20240)
    return _SD[cfg.name]


def _check(lib, cfg, prec, kset, B, mask_form="ones", uncond=False):
    """One forward of batch B on `kset`, all B x T rows against the bound; the oracle outputs are computed once per input and shared."""
    sd = _sd(cfg)
    x, ts, y = rowcheck.case_inputs(cfg, B, mask_form)
    m = DSGDenoiser(cfg, precision=prec, max_batch=B, library=lib).set_kernel_set(kset)
    m.load_state_dict(sd)
    out = np.asarray(m(x, ts, y, uncond_info=uncond))
    assert m.last_kernel_set() == kset
    outs = []
    for kind in ("fp32", rowcheck.ref_kind(prec, kset)):
        key = (cfg.name, B, mask_form, uncond, kind)
        if key not in _WANT:
            _WANT[key] = rowcheck.oracle(cfg, sd, kind)(x, [int(t) for t in ts], y, uncond_info=uncond)
            _WANT[key].setflags(write=False)
        outs.append(_WANT[key])
    worst = rowcheck.assert_rows_within(out, outs[0], outs[1], rowcheck.MARGIN[prec], f"{cfg.name} {prec} {kset} batch {B} {mask_form}")
    print(f"{cfg.name} {prec} {kset} batch {B} {mask_form}{' uncond' if uncond else ''}: worst row at {worst:.2f} x its reference error")
    return worst


@pytest.mark.parametrize("name,prec", sorted(SETS))
def test_every_row_of_every_clip_at_the_tiny_dims(emu_lib, name, prec):
    """Variants 3 / 4 / 5, bf16 and bf16w2, every kernel set the handle accepts: batch 3 and 5 (69 / 115 token rows at 23 per clip, 93 / 155 at 31:
    a ragged last 16-row tile and clip boundaries inside tiles each time), all rows within 2 x the rounded oracle's error of that row.  Measured
    under the emulator: worst rows at 1.0 ... 1.4 x."""
    cfg = C.CONFIGS[name]
    for kset in SETS[name, prec]:
        for B in (3, 5):
            _check(emu_lib, cfg, prec, kset, B)


def test_every_row_with_full_tiles_only(emu_lib):
    """Batch 16 at the tiny dims is 368 token rows = 23 full tiles (no ragged tail) on the two 16-row-tile sets."""
    for prec, kset in (("bf16", "rows"), ("bf16w2", "rows"), ("bf16", "tile")):
        _check(emu_lib, C.TINY, prec, kset, 16)


@pytest.mark.parametrize("name,prec,kset", [("tiny", "bf16", "rows"), ("tiny", "bf16", "stream"), ("tiny", "bf16w2", "rows"), ("tiny4", "bf16", "block"),
                                            ("tiny5", "bf16w2", "tile"), ("tiny", "fp32", "block")])
def test_every_row_with_a_per_clip_mask_and_without_a_mask(emu_lib, name, prec, kset):
    """mask_local per clip ([B, T]: clip b cut at its own length inside a window, the windows behind the cut masked entirely, a hole of three
    frames) and mask_local=None, batch 3: the masked windows are rows like the others (the oracle's softmax is uniform there, and finite)."""
    for mask_form in ("perclip", "none"):
        _check(emu_lib, C.CONFIGS[name], prec, kset, 3, mask_form)


@pytest.mark.parametrize("name,prec,kset", [("tiny", "bf16", "rows"), ("tiny4", "bf16", "block"), ("tiny5", "bf16w2", "tile")])
def test_every_row_of_the_unconditional_evaluation(emu_lib, name, prec, kset):
    """uncond_info=True (style embedding zeroed; variant 3: the seed zeroed before embed_text) against the oracles' unconditional branch."""
    _check(emu_lib, C.CONFIGS[name], prec, kset, 3, uncond=True)
