"""CPU: per-element noise streams (dsg_set_noise_streams / dsg_noise_streams; `clip_streams=` of the loops, `clip_ids=` of the clip drivers)
through the product sources under the SIMT emulator.  With them a clip's noise is the noise it gets sampled alone with its (seed, stream id),
so its result does not depend on the batch, slot or lane it rides in -- every comparison below is bit for bit.  The checks themselves are
tests/noise_streams_util.py; the real-hardware run is tests/test_gpu_noise_streams.py (-m gpu), the sharded one
tests/test_parallel_noise_streams.py."""
import pytest

from diffusestylegesture_amd import config as C
from tests import noise_streams_util as U


def test_noise_streams_tensor_vs_single_streams_and_oracle(emu_lib):
    U.check_noise(emu_lib)


@pytest.mark.parametrize("cfg,prec", [(C.TINY, "fp32"), (C.TINY, "bf16"), (C.TINY, "bf16w2"), (C.TINY4, "fp32"), (C.TINY4, "bf16")],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_slot_invariance_every_kernel_set(emu_lib, cfg, prec):
    """p_sample_loop and ddim_sample_loop (eta 0.5) on B = 3, shared seed and per-element seeds, under every kernel set the handle accepts
    at these dims for batch 3 and batch 1"""
    sets = U.accepted_sets(emu_lib, cfg, prec, 3)
    assert "tile" in sets and (prec == "bf16w2" or len(sets) >= 3), sets
    for ks in sets:
        for ddim, seeds in ((False, None), (True, U.SEEDS)):
            U.check_slot_invariance(emu_lib, cfg, prec, ks, ddim=ddim, seeds=seeds)


@pytest.mark.parametrize("variant,cfg,ddim", [("init", C.TINY, False), ("init", C.TINY4, True), ("inpaint", C.TINY, True),
                                              ("inpaint", C.TINY4, False), ("guided", C.TINY5, False), ("guided", C.TINY5, True),
                                              ("const", C.TINY, False)], ids=lambda v: v if isinstance(v, str) else getattr(v, "name", str(v)))
def test_slot_invariance_variants(emu_lib, variant, cfg, ddim):
    """init_image + skip_timesteps (the q_sample draw), a window-level inpainting constraint, fused guidance (max_batch 6) and const_noise
    (element 0's stream for everyone), bf16 and fp32, TILE named on both sides"""
    for prec, seeds in (("bf16", U.SEEDS), ("fp32", None)):
        U.check_slot_invariance(emu_lib, cfg, prec, "tile", variant=variant, ddim=ddim, seeds=seeds)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_arrangement_invariance_1x4_2x2_4x1(emu_lib, prec):
    U.check_arrangements(emu_lib, C.TINY, prec, "tile")


@pytest.mark.parametrize("cfg,prec", [(C.TINY, "bf16"), (C.TINY4, "fp32")], ids=lambda v: v if isinstance(v, str) else v.name)
def test_whole_clips_host_library_and_alone(emu_lib, cfg, prec):
    """generate_clip / generate_clip_dsgplus with clip_ids: host windows == library windows == the three batch-1 clips; plain, with
    init_motion (k_clip_x_in) and with a clip-level constraint; K = 2 and 3"""
    U.check_whole_clips(emu_lib, cfg, prec, "tile")


def test_off_is_off_and_clone_starts_unkeyed(emu_lib):
    U.check_off_is_off(emu_lib, C.TINY, "bf16", "tile")


def test_generators_own_their_streams(emu_lib):
    U.check_generators(emu_lib, C.TINY, "fp32", "tile")


def test_errors(emu_lib):
    U.check_errors(emu_lib, C.TINY)


def test_shard_clip_ids():
    from diffusestylegesture_amd.parallel import shard_clip_ids, shard_clips
    assert shard_clip_ids(4, 0, 1) == [[0, 1, 2, 3]] and shard_clip_ids(4, 1, 2) == [[1, 3]]
    assert shard_clip_ids(16, 1, 2, lanes=4) == [[1, 3], [5, 7], [9, 11], [13, 15]]
    assert sum(shard_clip_ids(16, 1, 2, lanes=4), []) == shard_clips(16, 1, 2)
    with pytest.raises(ValueError):
        shard_clip_ids(6, 0, 2, lanes=2)
