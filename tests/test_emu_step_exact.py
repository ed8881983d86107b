"""CPU, under the SIMT emulator: the one-step check of tests/stepcheck.py against the product sources compiled by the host compiler -- the tiny
dims in every kernel set that accepts them, in fp32, bf16 and bf16w2.  The case structure is that of tests/test_gpu_step_exact.py (A: the last
DDPM step is the forward; B: every element of one step; C: two steps in one call; D: draw_base and lanes), cut down to a few seconds per case:
each (dims, precision, set) runs every other mode at ONE loop index, and both move on with the case, so that all modes and all mode x index
pairs are met over the sets.  This proves the plumbing and the bound before any GPU time is spent."""
import numpy as np
import pytest

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.model import DSGDenoiser
from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
from tests import stepcheck as S

SETS = [("tiny", "bf16", ks) for ks in ("latency", "tile", "block", "rows", "stream")] + [("tiny", "bf16w2", ks) for ks in ("latency", "tile", "rows")] + \
       [("tiny", "fp32", ks) for ks in ("latency", "tile", "block")] + [("tiny4", "bf16", "block"), ("tiny5", "bf16", "tile"), ("tiny5", "bf16w2", "latency")]
GUIDED = [("tiny", "bf16", "tile"), ("tiny", "bf16", "block"), ("tiny", "bf16", "stream"), ("tiny", "fp32", "block"), ("tiny5", "bf16", "block")]
_SD = {}


def _case(lib, dims, prec, kset, B, guided=False, inpaint=False):
    cfg = C.CONFIGS[dims]
    if dims not in _SD:
        _SD[dims] = synth_state_dict(cfg, 20240)
    m = DSGDenoiser(cfg, precision=prec, max_batch=2 * B if guided else B, library=lib).set_kernel_set(kset)
    m.load_state_dict(_SD[dims])
    y = synth_window_inputs(cfg, B, window=1, clip0=3, seed_pose_scale=0.2)
    mask = motion = None
    if inpaint:
        r = np.random.RandomState(77)
        shape = (B, cfg.njoints, 1, cfg.n_poses)
        mask = np.zeros(shape, bool)
        mask[:, :cfg.njoints // 2] = r.rand(B, cfg.njoints // 2, 1, cfg.n_poses) < 0.5
        motion = (1.5 * r.randn(*shape)).astype(np.float32)
    scale = np.asarray([0.5, 1.0, 0.0, 2.5, 1.75][:B], np.float32) if guided else None
    return S.Case(m, kset, B, y, scale=scale, mask=mask, motion=motion, tag=f"{dims} {prec} {kset} {B}" + (" guided" if guided else ""))


@pytest.mark.parametrize("dims,prec,kset", SETS, ids=lambda v: str(v))
def test_a_and_b_at_the_tiny_dims(emu_lib, dims, prec, kset):
    """Batch 3 (69 / 93 token rows: a ragged last tile, clip boundaries inside tiles): A, then B for every other mode at one loop index each."""
    c = _case(emu_lib, dims, prec, kset, 3)
    c.check_last_step_is_forward()
    off = SETS.index((dims, prec, kset))
    worst = {}
    for k, m in enumerate(c.modes()):
        if (k + off) % 2:            # every other mode per case; the neighbouring case takes the others
            continue
        worst.update(c.check_all(indices=lambda n: (S.loop_indices(n)[(k + off) % 4],), modes=[m]))
    print(f"STEPCHECK (emulator) {c.tag}: worst element / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dims,prec,kset", GUIDED, ids=lambda v: str(v))
def test_guided_with_inpainting(emu_lib, dims, prec, kset):
    """3 clips + 3 twins, scales 0.5 / 1.0 / 0, a per-element constraint on half the joints whose motion reaches beyond +-1: A (unconstrained),
    B with the clamp on (select, then clamp) and off, C (the twin rows feed the second step)."""
    c = _case(emu_lib, dims, prec, kset, 3, True, True)
    c.check_last_step_is_forward()
    modes = [m for m in S.MODES if m[0] in ("ddpm-clip", "ddim-eta0.5-clip")]
    worst = {}
    for k, m in enumerate(modes):
        worst.update(c.check_all(indices=lambda n: (S.loop_indices(n)[(k + 1) % 4],), modes=[m]))
    worst["second of two"] = c.check_two_steps("ddpm", S.DDPM, "ddpm", {})
    print(f"STEPCHECK (emulator) {c.tag}: worst element / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("prec,kset", [("bf16", "latency"), ("bf16", "tile"), ("bf16", "block"), ("bf16", "rows"), ("bf16", "stream"), ("bf16w2", "rows"), ("fp32", "tile")])
def test_c_two_steps_in_one_call(emu_lib, prec, kset):
    c = _case(emu_lib, "tiny", prec, kset, 3)
    for name, mode, sched, args in S.MODES:
        if name in ("ddpm-clip", "ddim-eta1"):
            c.check_two_steps(name, mode, sched, args)


def test_d_draw_base_and_lanes(emu_lib):
    c = _case(emu_lib, "tiny", "bf16", "tile", 2)
    i = S.loop_indices(1000)[1]
    c.check("ddpm draw_base 7", S.DDPM, "ddpm", i, {}, seed=41, stream_id=9, draw_base=7)
    lanes = [c.model, c.model.clone()]
    ys = [synth_window_inputs(c.model.cfg, 2, window=k, clip0=2 * k, seed_pose_scale=0.2) for k in range(2)]
    x_ts = [np.random.RandomState(300 + k).randn(*c.shape).astype(np.float32) for k in range(2)]
    sids = [3, 2 ** 33 + 5]
    outs = S.lanes_one_step(lanes, c.diff["ddpm"], S.DDPM, i, x_ts, ys, seeds=[41, 41], stream_ids=sids, draw_base=7)
    for k, ln in enumerate(lanes):
        want, terms, _ = S.expected(ln, c.odiff["ddpm"], S.DDPM, i, x_ts[k], ys[k], seed=41, stream_id=sids[k], draw_base=7)
        S.assert_step_exact(outs[k], want, terms, f"lane {k} (stream_id {sids[k]})")
