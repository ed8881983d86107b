"""CPU, gloo: clips sharded over ranks draw the same noise on every world size (`parallel.shard_clip_ids` + `clip_ids=` of the clip drivers).
Four TINY clips sampled by one process as a batch of 4 and by two ranks as a batch of 2 each gather to the same [4, F, J] array, bit for bit
-- clip c is stream c wherever it rides.  The emulated product library, one kernel set named everywhere; in the style of
tests/test_parallel_gloo.py."""
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from diffusestylegesture_amd import config as C
from diffusestylegesture_amd.parallel import gather_poses, shard_clip_ids
from tests.conftest import EMU_LIB

N_CLIPS, K = 4, 2


def _clips(ids):
    """the clips `ids` as ONE batch: every clip its own conditioning, clip c on stream c"""
    from diffusestylegesture_amd import lib as L
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.sample import generate_clip
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    lib = L.DSGLibrary(EMU_LIB)
    cfg = C.TINY
    m = DSGDenoiser(cfg, precision="fp32", max_batch=len(ids), library=lib).set_kernel_set("tile")
    m.load_state_dict(synth_state_dict(cfg, 3))
    feats = [synth_window_inputs(cfg, len(ids), window=w, clips=ids)["audio"] for w in range(K)]
    return generate_clip(m, create_gaussian_diffusion(library=lib), feats, [1, 0, 0, 0, 0, 0], seed=7, skip_timesteps=997, clip_ids=ids)


def _worker(rank, world, port, q):
    os.environ["DSG_EMU_THREADS"] = "2"
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    mine = _clips(shard_clip_ids(N_CLIPS, rank, world)[0])
    dist.barrier()
    out = gather_poses(mine, N_CLIPS, dist, dst=0)
    if rank == 0:
        q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_of_two_clips_match_one_batch_of_four(emu_lib):
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = gather_poses(_clips(shard_clip_ids(N_CLIPS, 0, 1)[0]), N_CLIPS)      # world size 1: all four as one batch
    assert got.shape == ref.shape == (N_CLIPS, K * C.TINY.stride - C.TINY.n_seed, C.TINY.njoints)
    assert np.array_equal(got, ref)
    assert len({ref[c].tobytes() for c in range(N_CLIPS)}) == N_CLIPS
