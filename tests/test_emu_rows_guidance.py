"""CPU, under the SIMT emulator: classifier-free guidance fused into the ROWS set at the DSG+ widths (the guided streaming pose head k_ws_cfg,
dsg_stream.h) -- one guided forward at the BEAT++ dims, and what an explicit set / `auto` do with guided and unguided calls.  The GPU file
(tests/test_gpu_rows_guidance.py) has the batches, the per-row bound, the chains, inpainting and lanes."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.model import ClassifierFreeSampleModel, DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.util import rel_l2


def test_guided_forward_in_rows_at_beatpp_dims(emu_lib):
    """B = 1 (+ its twin, 302 rows: the conditional / twin boundary lies inside row tile 9 and inside the last 32-row block of the pose head) at the
    BEAT++ dims (variant 5, latent 384) in ROWS against uncond + s (cond - uncond) of the oracle's two evaluations, at the bf16 forward bound.
    Without the guided pose head the call raises NotImplementedError."""
    from oracle import sampler
    from oracle.mdm import MDMOracle
    cfg = C.BEATPP
    sd = synth_state_dict(cfg, 20240)
    y = dict(synth_window_inputs(cfg, 1, window=1, seed_pose_scale=0.2), scale=np.asarray([2.5], np.float32))
    x = np.random.RandomState(3).randn(1, cfg.njoints, 1, cfg.n_poses).astype(np.float32)
    m = DSGDenoiser(cfg, precision="bf16", max_batch=2, library=emu_lib).set_kernel_set("rows")
    m.load_state_dict(sd)
    out = np.asarray(ClassifierFreeSampleModel(m)(x, np.array([417]), y))
    assert m.last_kernel_set() == "rows"
    e = rel_l2(out, sampler.CFGModel(MDMOracle(sd, cfg))(x, [417], y))
    print(f"ROWS guidance beatpp 1 + 1 (emulator): rel-L2 {e:.3e}")
    assert e < 1.2e-2


@pytest.mark.parametrize("name", ["beat", "twh"])
def test_explicit_rows_is_accepted_and_auto_is_unchanged(emu_lib, name):
    """ROWS is accepted on a DSG+ handle (and can no longer fail at the first guided call); what `auto` resolves to is what it was -- the lists of the
    round-6 tests for unguided calls, BLOCK (TILE below 600 rows in one lane / 300 per lane) for a handle whose conditioning is guided.  The
    conditioning alone decides: set_cond runs no kernel."""
    cfg = C.CONFIGS[name]
    m = DSGDenoiser(cfg, precision="bf16", max_batch=2, library=emu_lib)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    wide = "rows" if cfg.latent_dim == 384 else "block"
    unguided = lambda: ([m.recommend_kernel_set(b, 1) for b in (4, 8, 9, 13, 16, 27, 28, 48)], [m.recommend_kernel_set(b, 4) for b in (2, 3, 4, 8)])
    want = (["block", "block", wide, "rows", "rows", "rows", "rows", "rows"], ["block", "block", "rows", "rows"])
    assert unguided() == want
    y = synth_window_inputs(cfg, 1, window=1, seed_pose_scale=0.2)
    m.set_cond(y, 1, cfg_scale=np.asarray([1.5], np.float32))
    assert [m.recommend_kernel_set(b, 1) for b in (1, 3, 4, 8, 9, 13, 16, 48)] == ["tile", "tile", "block", "block", "block", "block", "block", "block"]
    assert [m.recommend_kernel_set(b, 4) for b in (1, 2, 3, 4, 8)] == ["tile", "block", "block", "block", "block"]
    m.set_cond(y, 1)
    assert unguided() == want
    assert m.set_kernel_set("rows").kernel_set() == "rows"
    with pytest.raises(NotImplementedError):
        DSGDenoiser(cfg, precision="fp32", max_batch=2, library=emu_lib).set_kernel_set("rows")
