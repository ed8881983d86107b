"""MI355X (-m gpu): per-element noise streams (dsg_set_noise_streams / dsg_noise_streams; `clip_streams=` of the loops, `clip_ids=` of the
clip drivers) on the real kernels -- the checks of tests/noise_streams_util.py, which the emulator runs in tests/test_emu_noise_streams.py,
under every kernel set the handle accepts, plus what only exists here: the generic (hooked) loop on device tensors, and the ROWS pose head
at the ZEGGS widths.  One kernel set is named for both sides of every comparison (LATENCY at batch 1 against TILE at batch 3 is no valid
pair: sets differ in the last bits)."""
import ctypes

import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from tests import noise_streams_util as U
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TOL_HOOK_FP32 = 1e-4      # the fp32 chain bound of the hook tests, tests/test_gpu_round5.py (TOL_CHAIN["fp32"])


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


def test_noise_streams_tensor_vs_single_streams_and_oracle(gpu):
    U.check_noise(gpu)


@pytest.mark.parametrize("cfg,prec", [(C.TINY, "fp32"), (C.TINY, "bf16"), (C.TINY, "bf16w2"), (C.TINY4, "bf16")],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_slot_invariance_every_kernel_set(gpu, cfg, prec):
    sets = U.accepted_sets(gpu, cfg, prec, 3)
    print("kernel sets:", sets)
    assert "tile" in sets
    for ks in sets:
        for ddim, seeds in ((False, None), (True, U.SEEDS)):
            U.check_slot_invariance(gpu, cfg, prec, ks, ddim=ddim, seeds=seeds)


@pytest.mark.parametrize("variant,cfg,ddim", [("init", C.TINY, False), ("init", C.TINY4, True), ("inpaint", C.TINY, True),
                                              ("inpaint", C.TINY4, False), ("guided", C.TINY5, False), ("guided", C.TINY5, True),
                                              ("const", C.TINY, False)], ids=lambda v: v if isinstance(v, str) else getattr(v, "name", str(v)))
def test_slot_invariance_variants(gpu, variant, cfg, ddim):
    for prec, seeds in (("bf16", U.SEEDS), ("fp32", None)):
        U.check_slot_invariance(gpu, cfg, prec, "tile", variant=variant, ddim=ddim, seeds=seeds)


def test_slot_invariance_zeggs_rows(gpu):
    """the streaming pose head (k_ws<EPI_OUT>) exists only at the product widths: batch 3, 4 steps, bf16, ROWS named on both sides"""
    U.check_slot_invariance(gpu, C.ZEGGS, "bf16", "rows", ddim=False, seeds=U.SEEDS)


def test_arrangement_invariance_1x4_2x2_4x1(gpu):
    U.check_arrangements(gpu, C.TINY, "bf16", "tile")


@pytest.mark.parametrize("cfg", [C.TINY, C.TINY4], ids=lambda c: c.name)
def test_whole_clips_host_library_and_alone(gpu, cfg):
    U.check_whole_clips(gpu, cfg, "bf16", "tile")


def test_hooked_loop_draws_the_same_streams(gpu, monkeypatch):
    """An identity `denoised_fn` sends the loop through the generic path (the denoiser through the library, the update kernels of the library,
    the noise through dsg_noise_streams): it agrees with the fused loop under the same `clip_streams` within the fp32 chain bound of the hook
    tests, and the noise it asks for -- every dsg_noise_streams call is recorded and repeated into host memory -- is, element by element, the
    batch-1 tensor of that element's (seed, stream id) at draw 0 (x_T) and 1 + i (step i)."""
    import torch
    cfg, B = C.TINY, 3
    shape = (B, cfg.njoints, 1, cfg.n_poses)
    m, d = U.model(gpu, cfg, "fp32", B, "tile"), U.diffusion(gpu)
    y = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in U.y_of(cfg, U.CLIPS).items()}
    streams = U.pairs(U.SEEDS, U.STREAMS)
    real, seen = gpu.cdll.dsg_noise_streams, []

    def recorder(out, b, j, t, seeds, ids, draw, stream):
        host = np.zeros((b, j, 1, t), np.float32)
        assert real(host.ctypes.data, b, j, t, seeds, ids, draw, None) == 0
        seen.append((int(draw), host))
        return real(out, b, j, t, seeds, ids, draw, stream)
    for ddim in (False, True):
        fused = U.loop(d.manual_seed(1, 0), ddim)(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=U.SKIP, clip_streams=streams)
        del seen[:]
        monkeypatch.setattr(gpu.cdll, "dsg_noise_streams", recorder)
        hooked = U.loop(d.manual_seed(1, 0), ddim)(m, shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=U.SKIP,
                                                   clip_streams=streams, denoised_fn=lambda x0: x0)
        monkeypatch.setattr(gpu.cdll, "dsg_noise_streams", real)
        err = rel_l2(hooked.cpu().numpy(), fused.cpu().numpy())
        print(f"hooked vs fused loop, ddim={ddim}: rel-L2 {err:.3e} (bound {TOL_HOOK_FP32})")
        assert err < TOL_HOOK_FP32
        assert [dr for dr, _ in seen] == [0, 1, 2, 3, 4] and d._draw == 5
        for dr, z in seen:
            for b in range(B):
                assert np.array_equal(z[b:b + 1], U.noise_alone(gpu, cfg.njoints, cfg.n_poses, U.SEEDS[b], U.STREAMS[b], dr)), (ddim, dr, b)


def test_off_is_off_and_clone_starts_unkeyed(gpu):
    U.check_off_is_off(gpu, C.TINY, "bf16", "tile")


def test_generators_own_their_streams(gpu):
    U.check_generators(gpu, C.TINY, "bf16", "tile")


def test_errors(gpu):
    U.check_errors(gpu, C.TINY)
