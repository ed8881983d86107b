"""CPU, under the SIMT emulator: the ROWS kernel set in bf16w2 at the DSG+ widths (latent_dim 384 / 512) -- per layer the QKV GEMM on the hi + lo
rows in X0a (k_gemm_qkv_pair), k_attn and k_ffn<OP> on one 16-row tile with two-register fragments (W_o leading the ring, operand fragments re-read
from LDS).  Batch 2 is 302 token rows: 18 tiles + 14 rows, the clip boundary inside tile 9.  tests/test_gpu_rows_w2_wide.py has batch 3, the masks,
the other DSG+ configs, the step checks and the chains on the device."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.model import ClassifierFreeSampleModel, DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests import rowcheck

_SD, _RUN = {}, {}


def _sd(cfg):
    if cfg.name not in _SD:
        _SD[cfg.name] = synth_state_dict(cfg, 20240)
    return _SD[cfg.name]


def _model(lib, cfg, kset, max_batch):
    m = DSGDenoiser(cfg, precision="bf16w2", max_batch=max_batch, library=lib).set_kernel_set(kset)
    m.load_state_dict(_sd(cfg))
    return m


def _forward_b2(lib, name):
    """(inputs, output) of the batch-2 ROWS forward of one config: run once, shared by the two tests that read it, read-only."""
    if name not in _RUN:
        cfg = C.CONFIGS[name]
        x, ts, y = rowcheck.case_inputs(cfg, 2)
        m = _model(lib, cfg, "rows", 2)
        out = np.asarray(m(x, ts, y))
        assert m.last_kernel_set() == "rows"
        out.setflags(write=False)
        _RUN[name] = ((x, ts, y), out)
    return _RUN[name]


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_every_row_of_a_rows_forward(emu_lib, name):
    """One forward of batch 2 on the pinned set: every (clip, frame) row within 2 x its reference error, the reference being the oracle with the
    bf16w2 roundings of ROWS (the embedding output a hi + lo pair like the other A operands)."""
    cfg = C.CONFIGS[name]
    (x, ts, y), out = _forward_b2(emu_lib, name)
    worst = rowcheck.assert_every_row(out, x, ts, y, cfg, _sd(cfg), "bf16w2", kset="rows")
    print(f"ROWCHECK {name} bf16w2 rows batch 2 (emulator): worst row at {worst:.2f} x its reference error")


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_a_clip_does_not_depend_on_its_batch(emu_lib, name):
    """Clip 1 of the batch-2 output (token rows 151 .. 301: it starts inside tile 9) is bit for bit the batch-1 output of a second handle with that
    clip's inputs."""
    cfg = C.CONFIGS[name]
    (x, ts, y), out = _forward_b2(emu_lib, name)
    y1 = {k: (np.asarray(v)[1:2] if v is not None and np.asarray(v).shape[0] == 2 else v) for k, v in y.items()}
    m = _model(emu_lib, cfg, "rows", 1)
    one = np.asarray(m(x[1:2], ts[1:2], y1))
    assert m.last_kernel_set() == "rows"
    assert np.array_equal(one[0], out[1])


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_auto_still_resolves_to_tile(emu_lib, name):
    """DSG_KSET_AUTO is untouched: TILE at every batch and lane count, and a forward under `auto` runs TILE."""
    cfg = C.CONFIGS[name]
    m = _model(emu_lib, cfg, "auto", 1)
    assert [m.recommend_kernel_set(b, 1) for b in (1, 8, 16, 48)] == ["tile"] * 4
    assert [m.recommend_kernel_set(b, 4) for b in (1, 4, 16)] == ["tile"] * 3
    x, ts, y = rowcheck.case_inputs(cfg, 1)
    assert np.isfinite(np.asarray(m(x, ts, y))).all()
    assert m.last_kernel_set() == "tile"


def test_what_stays_refused(emu_lib):
    """Fused guidance on the ROWS-pinned bf16w2 handle, and bf16w2 in BLOCK / STREAM, are NotImplementedError as before."""
    cfg = C.BEAT
    m = _model(emu_lib, cfg, "rows", 2)
    y = dict(synth_window_inputs(cfg, 1, window=1, seed_pose_scale=0.2), scale=np.asarray([2.5], np.float32))
    x = np.random.RandomState(3).randn(1, cfg.njoints, 1, cfg.n_poses).astype(np.float32)
    with pytest.raises(NotImplementedError):
        ClassifierFreeSampleModel(m)(x, np.array([417]), y)
    for kset in ("block", "stream"):
        with pytest.raises(NotImplementedError):
            m.set_kernel_set(kset)
    assert m.kernel_set() == "rows"
