"""MI355X (-m gpu): a whole clip per library call (dsg_sample_clip, `windows="library"`): the window hand-off kernel at the product widths --
J = 1141 / 2052 / 2232, where a stitched row starts on any 4-byte boundary -- bit for bit against the host window loop (`windows="host"`) on
the same handle under the same kernel set; several lanes; the oracle's inference() loop; and the kernel alone against a numpy restatement
of the stitch.  The emulator tests are tests/test_emu_clip.py."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TOL_CHAIN_BF16 = 2e-2      # the bf16 chain bound of the GPU suite: tests/test_gpu_round3.py:23 (TOL_CHAIN["bf16"])
K, N_RUN = 3, 4
SKIP = 1000 - N_RUN


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from diffusestylegesture_amd import lib as L
    return L.default_library()


def _model(cfg, B, kset=None):
    from diffusestylegesture_amd.model import DSGDenoiser
    m = DSGDenoiser(cfg, precision="bf16", max_batch=B, device=0)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    return m.set_kernel_set(kset) if kset else m


def _inputs(cfg, B, clip0=0):
    import torch
    ins = [synth_window_inputs(cfg, B, window=w, clip0=clip0, seed_pose_scale=0.2) for w in range(K)]
    return ins, [torch.from_numpy(y["audio"]).cuda() for y in ins]


def _clip(cfg, m, d, ins, feats, windows, skip=SKIP, stream_id=0):
    import torch
    from diffusestylegesture_amd.sample import generate_clip, generate_clip_dsgplus
    style = [1] + [0] * (cfg.style_dim_in - 1)
    if cfg is C.ZEGGS:
        return generate_clip(m, d, feats, style, seed=31, smoothing=True, skip_timesteps=skip, stream_id=stream_id, windows=windows)
    return generate_clip_dsgplus(m, d, feats, style, torch.from_numpy(ins[0]["seed"]).cuda(), K * cfg.stride, seed=31, skip_timesteps=skip,
                                 stream_id=stream_id, feature_division=1, windows=windows)


@pytest.mark.parametrize("cfg,B,kset", [(C.ZEGGS, 3, None), (C.BEAT, 2, None), (C.TWH, 1, None), (C.ZEGGS, 16, "rows")],
                         ids=["zeggs-b3", "beat-b2", "twh-b1", "zeggs-b16-rows"])
def test_library_windows_bit_identical_to_host_loop(gpu, cfg, B, kset):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    m, d = _model(cfg, B, kset), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    host = _clip(cfg, m, d, ins, feats, "host")
    path, ks, draw = m.last_sample_path(), m.last_kernel_set(), d._draw
    lib = _clip(cfg, m, d, ins, feats, "library")
    assert host.shape == lib.shape == (B, K * cfg.stride - (cfg.n_seed if cfg is C.ZEGGS else 0), cfg.njoints)
    assert np.isfinite(lib).all() and np.array_equal(host, lib)
    assert m.last_sample_path() == path and m.last_kernel_set() == ks and (kset is None or ks == kset)
    assert d._draw == draw == K * (1 + N_RUN) and m.last_sample_ms()[1] == K * N_RUN
    assert B == 1 or not np.array_equal(lib[0], lib[1])


def test_lanes_bit_identical_to_host_form(gpu):
    """generate_clips_streams(..., windows="library"), 2 lanes x 2 clips"""
    import torch
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.sample import generate_clips_streams
    cfg, NL, B = C.ZEGGS, 2, 2
    m = _model(cfg, B)
    lanes, d = [m, m.clone()], create_gaussian_diffusion()
    feats = [_inputs(cfg, B, clip0=ln * B)[1] for ln in range(NL)]
    run = lambda w: generate_clips_streams(lanes, d, feats, [0, 1, 0, 0, 0, 0], seed=17, skip_timesteps=SKIP, stream_ids=[5, 6], windows=w)
    host = run("host")
    paths = [ln.last_sample_path() for ln in lanes]
    lib = run("library")
    assert host.shape == (NL * B, K * cfg.stride - cfg.n_seed, cfg.njoints) and np.array_equal(host, lib)
    assert [ln.last_sample_path() for ln in lanes] == paths and not np.array_equal(lib[:B], lib[B:])


def test_zeggs_clip_vs_oracle(gpu):
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from oracle import philox, sampler
    from oracle.mdm import MDMOracle
    from oracle.schedule import OracleDiffusion
    cfg, B, b, sid = C.ZEGGS, 2, 1, 4
    m, d = _model(cfg, B), create_gaussian_diffusion()
    ins, feats = _inputs(cfg, B)
    got = _clip(cfg, m, d, ins, feats, "library", stream_id=sid)
    ref, od = MDMOracle(synth_state_dict(cfg, 20240), cfg), OracleDiffusion()
    shape = (B, cfg.njoints, 1, cfg.n_poses)

    def sample_window(c, y):
        nf = lambda k: philox.normal_bj1t(shape, 31, c * (1 + N_RUN) + k, sid)[b:b + 1]
        return sampler.p_sample_loop(od, ref, (1,) + shape[1:], nf, {"y": y}, skip_timesteps=SKIP)
    want = sampler.zeggs_clip(sample_window, cfg, [y["audio"][b:b + 1] for y in ins], [1, 0, 0, 0, 0, 0])
    e = rel_l2(got[b], want)
    print(f"library clip (ZEGGS, K = {K}, {N_RUN} steps) vs oracle.sampler.zeggs_clip: rel-L2 {e:.3e}")
    assert e < TOL_CHAIN_BF16


@pytest.mark.parametrize("cfg,B", [(C.ZEGGS, 2), (C.BEAT, 1)], ids=["zeggs", "beat"])
def test_handoff_kernel_alone_vs_numpy_stitch(gpu, cfg, B):
    """one step per window: the clip call is the hand-off kernel and little else.  Yardstick: the K single-window samples of p_sample_loop,
    stitched by a numpy restatement of sample.py:269-289 / BEAT-TWH sample.py:150-160 (fp32, the same operations in the same order)."""
    import torch
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    m, d = _model(cfg, B), create_gaussian_diffusion()
    skip = d.num_timesteps - 1
    ins, feats = _inputs(cfg, B)
    zeggs = cfg is C.ZEGGS
    Sd, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
    got = _clip(cfg, m, d, ins, feats, "library", skip=skip)
    d.manual_seed(31, 0)
    style = np.repeat(np.asarray([[1] + [0] * (cfg.style_dim_in - 1)], np.float32), B, 0)
    tail = np.zeros((B, J, 1, Sd), np.float32) if zeggs else ins[0]["seed"]
    rows = []                                  # frame-major pieces [B, frames, J]
    for c in range(K):
        y = {"style": style, "seed": np.ascontiguousarray(tail), "audio": feats[c], "mask_local": np.ones((1, T), bool)}
        s = d.p_sample_loop(m, (B, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip).cpu().numpy()[:, :, 0, :]
        s = s.transpose(0, 2, 1).copy()        # [B, T, J]
        if c > 0:
            last0 = tail[:, :, 0, 0]           # frame 0 of the previous window's tail, [B, J]
            if zeggs:
                delta = s[:, 0, :3] - last0[:, :3]
                s[:, :, :3] = s[:, :, :3] - delta[:, None, :]
            s[:, 0] = last0 * np.float32(0.5) + s[:, 0] * np.float32(0.5)
        tail = s[:, T - Sd:].transpose(0, 2, 1)[:, :, None, :]
        rows.append(s if (c == K - 1 and not zeggs) else s[:, : T - Sd])
    want = np.concatenate(rows, 1)[:, Sd:]
    assert got.shape == want.shape and np.array_equal(got, want)
