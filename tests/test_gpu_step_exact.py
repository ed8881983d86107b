"""GPU: ONE denoising step of the fused sampler, every element of every clip against the float64 update formula at 8 u S (tests/stepcheck.py
has the bound and its derivation) -- in every pose-head kernel, bf16 included: the device's own forward supplies the step's x0 and dsg_noise
its noise, so the denoiser's bf16 drift is not in the comparison.  The cases are the smallest batches that reach each pose-head instantiation
and its ragged edges; the guided ones carry a per-clip scale (one clip at 1.0, one at 0) and the unconditional twins.
  A  the last DDPM step (k1 = 1, k2 = 0, no noise) returns forward(x_t, timestep_map[0]) bit for bit
  B  every element of one step, for every mode x loop index {0, middle, n - 2, n - 1} (1000-step DDPM, DDIM respaced to 50)
  C  two steps in one call == two one-step calls; the second step passes B with x0 = forward(out_1): state shadow, twin rows, pad columns
  D  draw bookkeeping: draw_base = 7 with first_step = i, and 4 lanes x 4 clips through dsg_sample_multi, each lane on its own stream_id"""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests import stepcheck as S

pytestmark = pytest.mark.gpu

# (dims, precision, kernel set, batch)
CASES = [("tiny", "bf16", "rows", 23), ("tiny", "bf16", "stream", 23), ("zeggs", "bf16", "latency", 1), ("zeggs", "bf16", "latency", 2),
         ("zeggs", "bf16", "tile", 3), ("zeggs", "bf16w2", "tile", 3), ("zeggs", "fp32", "tile", 3), ("zeggs", "bf16", "block", 12),
         ("zeggs", "fp32", "block", 12), ("zeggs", "bf16", "rows", 23), ("zeggs", "bf16w2", "rows", 16), ("zeggs", "bf16", "stream", 23),
         ("zeggs", "bf16", "stream", 48), ("beat", "bf16", "tile", 1), ("beat", "bf16", "block", 8), ("beat", "bf16", "rows", 9),
         ("twh", "bf16", "rows", 13), ("beatv2", "bf16", "rows", 9)]
# guided: (dims, precision, kernel set, clips (+ as many twins), inpainting)
GUIDED = [("zeggs", "bf16", "block", 6, False), ("zeggs", "bf16", "stream", 12, False), ("beat", "bf16", "rows", 9, False),
          ("twh", "bf16", "rows", 13, False), ("beat", "bf16", "block", 4, False), ("zeggs", "bf16", "block", 6, True)]
ONE_PER_SET = [("zeggs", "bf16", "latency", 2), ("zeggs", "bf16", "tile", 3), ("zeggs", "bf16", "block", 12), ("zeggs", "bf16", "rows", 23),
               ("zeggs", "bf16", "stream", 23)]
TWO_STEPS = ONE_PER_SET + [("zeggs", "fp32", "block", 12), ("zeggs", "bf16w2", "rows", 16), ("twh", "bf16", "rows", 13)]
_SD, _CASE = {}, {}


def _id(c):
    return "-".join(str(v) for v in c)


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


def _ext(n, shape, i, z):
    """step_noise of the whole chain in device memory, only slice i written (the step reads no other)."""
    import torch
    buf = torch.empty((n,) + tuple(shape), dtype=torch.float32, device="cuda:0")
    buf[i].copy_(torch.from_numpy(z))
    return buf


def scales(B):
    """y['scale'] per clip: linspace(0.5, 2.5) with clip 1 at 1.0 and the last but one at 0 (B = 4: clips 1 and 2)."""
    s = np.linspace(0.5, 2.5, B).astype(np.float32)
    s[1], s[B - 2] = 1.0, 0.0
    return s


def case(gpu, dims, prec, kset, B, guided=False, inpaint=False):
    """The case's model and inputs, built once and kept while the tests of that case run (one at a time: the previous one is released)."""
    from diffusestylegesture_amd.model import DSGDenoiser
    key = (dims, prec, kset, B, guided, inpaint)
    if key not in _CASE:
        _CASE.clear()
        cfg = C.CONFIGS[dims]
        m = DSGDenoiser(cfg, precision=prec, max_batch=2 * B if guided else B, device=0).set_kernel_set(kset)
        m.load_state_dict(_sd(cfg))
        y = synth_window_inputs(cfg, B, window=1, clip0=3, seed_pose_scale=0.2)
        mask = motion = None
        if inpaint:      # per element, on half the joints; the motion reaches beyond +-1, so select-then-clamp differs from clamp-then-select
            r = np.random.RandomState(77)
            shape = (B, cfg.njoints, 1, cfg.n_poses)
            mask = np.zeros(shape, bool)
            mask[:, :cfg.njoints // 2] = r.rand(B, cfg.njoints // 2, 1, cfg.n_poses) < 0.5
            motion = (1.5 * r.randn(*shape)).astype(np.float32)
        _CASE[key] = S.Case(m, kset, B, y, scale=scales(B) if guided else None, mask=mask, motion=motion, ext=_ext,
                            tag=f"{dims} {prec} {kset} {B}" + (f" + {B} twins" if guided else "") + (" inpainting" if inpaint else ""))
    return _CASE[key]


def _report(c, what, worst):
    print(f"STEPCHECK {c.tag} {what}: worst element / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dims,prec,kset,B", CASES, ids=[_id(c) for c in CASES])
def test_a_last_ddpm_step_is_the_forward(gpu, dims, prec, kset, B):
    case(gpu, dims, prec, kset, B).check_last_step_is_forward()


@pytest.mark.parametrize("dims,prec,kset,B,pos", [c + (pos,) for c in CASES for pos in range(4)],
                         ids=[_id(c) + "-" + p for c in CASES for p in ("first", "middle", "n-2", "last")])
def test_b_every_element_of_one_step(gpu, dims, prec, kset, B, pos):
    """`pos`: which of the loop indices {0, middle, n - 2, n - 1}; every mode of stepcheck.MODES at that index."""
    c = case(gpu, dims, prec, kset, B)
    _report(c, f"loop index #{pos}", c.check_all(indices=lambda n: (S.loop_indices(n)[pos],)))


@pytest.mark.parametrize("dims,prec,kset,B,inpaint", GUIDED, ids=[_id(c) for c in GUIDED])
def test_guided_a_b_c(gpu, dims, prec, kset, B, inpaint):
    """B clips + B twins, per-clip scale: A (without the constraint), B at every loop index for the modes that differ in the epilogue's
    guided path, C for DDPM and DDIM eta = 0.5 (the twin rows' state and shadow feed the second step)."""
    c = case(gpu, dims, prec, kset, B, True, inpaint)
    c.check_last_step_is_forward()
    modes = [m for m in c.modes() if m[0] in ("ddpm", "ddpm-clip", "ddpm-const", "ddpm50-ext", "ddim-eta0", "ddim-eta0.5-clip", "ddim-eta1")]
    _report(c, "guided", c.check_all(modes=modes))
    w = {name: c.check_two_steps(name, mode, sched, args) for name, mode, sched, args in S.MODES if name in ("ddpm", "ddim-eta0.5")}
    _report(c, "second of two steps", w)


@pytest.mark.parametrize("dims,prec,kset,B", TWO_STEPS, ids=[_id(c) for c in TWO_STEPS])
def test_c_two_steps_state_shadow_and_pad_columns(gpu, dims, prec, kset, B):
    c = case(gpu, dims, prec, kset, B)
    w = {name: c.check_two_steps(name, mode, sched, args) for name, mode, sched, args in S.MODES if name in ("ddpm", "ddpm-clip", "ddim-eta1")}
    _report(c, "second of two steps", w)


def test_d_draw_bookkeeping_and_lanes(gpu):
    """draw_base = 7 and first_step = i: the noise is draw 7 + 1 + i; then 4 lanes x 4 clips through dsg_sample_multi, every lane on its own
    stream_id, every lane passing B and bit-identical to the lane stepped alone."""
    c = case(gpu, "zeggs", "bf16", "tile", 4)
    n = 1000
    for i in (0, S.loop_indices(n)[1]):
        w = c.check("ddpm draw_base 7", S.DDPM, "ddpm", i, {}, seed=41, stream_id=9, draw_base=7)
        print(f"STEPCHECK {c.tag} draw_base 7, first_step {i}: worst element / bound {w:.3f}")
    w = c.check("ddim draw_base 7", S.DDIM, "ddim50", 20, {"eta": 1.0}, seed=41, stream_id=9, draw_base=7)
    print(f"STEPCHECK {c.tag} DDIM-50 draw_base 7, first_step 20: worst element / bound {w:.3f}")
    lanes = [c.model] + [c.model.clone() for _ in range(3)]
    for ln in lanes:
        ln.set_kernel_set("tile")
    i = S.loop_indices(n)[1]
    od = c.odiff["ddpm"]
    ys = [synth_window_inputs(c.model.cfg, 4, window=k, clip0=4 * k, seed_pose_scale=0.2) for k in range(4)]
    x_ts = [np.random.RandomState(300 + k).randn(*c.shape).astype(np.float32) for k in range(4)]
    sids = [3, 4, 11, 2 ** 33 + 5]
    outs = S.lanes_one_step(lanes, c.diff["ddpm"], S.DDPM, i, x_ts, ys, seeds=[41] * 4, stream_ids=sids, draw_base=7)
    for k, ln in enumerate(lanes):
        assert ln.last_kernel_set() == "tile"
        want, terms, _ = S.expected(ln, od, S.DDPM, i, x_ts[k], ys[k], seed=41, stream_id=sids[k], draw_base=7)
        w = S.assert_step_exact(outs[k], want, terms, f"lane {k} of 4 (stream_id {sids[k]})")
        alone = S.one_step(ln, c.diff["ddpm"], S.DDPM, i, x_ts[k], ys[k], seed=41, stream_id=sids[k], draw_base=7)
        assert np.array_equal(outs[k], alone), k
        print(f"STEPCHECK lane {k} of 4 x 4 clips, stream_id {sids[k]}: worst element / bound {w:.3f}")
