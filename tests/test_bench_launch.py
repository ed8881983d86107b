"""CPU: `python bench.py --gpus 2` must create two ranks ITSELF (no launcher environment), one per device, and report
n_gpus 2 -- exercised with the emulated library and gloo (DSG_BENCH_EMU=1: test infrastructure, tiny dims, a few denoising
steps); both multi-clip modes of config[3] (one clip per lane / one lock-step batch) go through the same code on one rank."""
import json
import os
import subprocess
import sys

from tests.conftest import ROOT


def _run(args, env_extra):
    env = dict(os.environ)
    env.update({"DSG_BENCH_EMU": "1", "DSG_BENCH_SKIP": "997", "DSG_EMU_THREADS": "2"})
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]        # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus2_spawns_two_ranks(emu_lib, tmp_path):
    """... and rank 0's gathered[c] IS clip c: bench.py deals clips with parallel.shard_clips (clip c -> rank c % world), the map
    gather_poses inverts, and a clip's inputs / Philox stream are functions of its id -- so every gathered row equals the same clip
    sampled by one process on one lane (round-3 verdict: the two used to disagree, block vs round-robin)."""
    import numpy as np
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.sample import generate_clip
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    dump = str(tmp_path / "dump")
    out = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--precision", "fp32", "--clips-per-gpu", "2", "--dump-outputs", dump], {})
    assert out["n_gpus"] == 2 and out["config"]["clips_per_gpu"] == 2 and out["config"]["mode"] == "streams"
    assert out["config"]["parallelism"] == "clips x2" and out["value"] > 0 and out["scaling"] == "weak"
    assert "EMULATED" in out["data"]
    got = np.load(os.path.join(dump, "poses.npy"))
    cfg = C.TINY
    assert got.shape[0] == 4
    m = DSGDenoiser(cfg, precision="fp32", max_batch=1, library=emu_lib)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    d = create_gaussian_diffusion(library=emu_lib)
    for c in range(4):
        feats = [synth_window_inputs(cfg, 1, window=w, clips=[c])["audio"] for w in range(2)]
        want = generate_clip(m, d, feats, [1] + [0] * (cfg.style_dim_in - 1), seed=123456, smoothing=True, stream_id=c, skip_timesteps=997)
        assert np.array_equal(got[c], want[0]), c


def test_bench_single_rank_modes(emu_lib):
    a = _run(["--steps", "1", "--warmup", "0", "--precision", "fp32", "--clips-per-gpu", "3", "--mode", "lockstep", "--no-cpu-baseline"], {})
    assert a["n_gpus"] == 1 and a["config"]["mode"] == "lockstep" and a["sample_path"] == "hip"
    b = _run(["--steps", "1", "--warmup", "0", "--precision", "fp32"], {})
    assert b["config"]["clips_per_gpu"] == 1 and b["roofline"]["bound"] == "hbm"
    assert b["value_emitted_frames"] < b["value"] and b["kernel_set"] == "tile" and "config3" not in b          # (fp32 at batch 1: TILE since round 5)
    # the config[3] sub-record the multi-GPU runs carry (16 clips per GPU as 4 lanes x batch 4), forced on one emulated rank
    c = _run(["--steps", "1", "--warmup", "0", "--precision", "fp32", "--config3", "on", "--no-cpu-baseline"], {"DSG_EMU_THREADS": "8", "DSG_BENCH_SKIP": "998"})
    assert c["config3"]["clips"] == 16 and c["config3"]["value"] > 0 and c["config3"]["kernel_set"] == "tile"


def test_bench_dump_outputs_is_the_last_timed_step(emu_lib, tmp_path):
    """`--dump-outputs DIR` writes the poses of the LAST of the `--steps` timed passes: pass i of the run samples with seed 123456 + i
    (warm-up passes first), so with --warmup 1 --steps 2 the dump is the clip sampled with seed 123458."""
    import numpy as np
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.sample import generate_clip
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    dump = str(tmp_path / "dump")
    out = _run(["--steps", "2", "--warmup", "1", "--precision", "fp32", "--no-cpu-baseline", "--dump-outputs", dump], {})
    assert out["steps"] == 2 and out["warmup"] == 1
    assert os.listdir(dump) == ["poses.npy"]
    got = np.load(os.path.join(dump, "poses.npy"))
    cfg = C.TINY
    m = DSGDenoiser(cfg, precision="fp32", max_batch=1, library=emu_lib)
    m.load_state_dict(synth_state_dict(cfg, 20240))
    d = create_gaussian_diffusion(library=emu_lib)
    feats = [synth_window_inputs(cfg, 1, window=w, clips=[0])["audio"] for w in range(2)]
    want = generate_clip(m, d, feats, [1] + [0] * (cfg.style_dim_in - 1), seed=123458, smoothing=True, stream_id=0, skip_timesteps=997)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_bench_plain_run_measures_only_the_headline():
    """A plain run measures nothing beyond its headline figure; `--full` adds what the line carried before the option existed (the
    config3 pass and the sub-records of the default workload, the .bvh post-processing, the CPU baseline), and the explicit switches
    still force or drop their parts -- decided by bench.extras, checked here for runs on the GPU and under the emulator."""
    import bench
    want = lambda argv, world=1, emu=False, variant=3: bench.extras(bench.parse(argv), world, emu, variant)
    none = {"config3": False, "sub_records": False, "postprocess": False, "cpu_baseline": False}
    assert want(["--gpus", "1", "--steps", "20", "--warmup", "5"]) == none
    assert want(["--gpus", "8", "--steps", "3"], world=8) == none
    assert want(["--clips-per-gpu", "16"]) == none
    assert want(["--full"]) == {k: True for k in none}
    assert want(["--full", "--gpus", "8"], world=8) == dict(none, config3=True, postprocess=True)
    assert want(["--full", "--clips-per-gpu", "16"]) == dict(none, postprocess=True, cpu_baseline=True)
    assert want(["--full", "--sampler", "ddim50"]) == dict(none, postprocess=True)
    assert want(["--full", "--config", "beat"], variant=4) == none
    assert want(["--full", "--sub-records", "off", "--no-cpu-baseline", "--no-postprocess"]) == none
    assert want(["--full", "--config3", "off"]) == dict(none, sub_records=True, postprocess=True, cpu_baseline=True)
    assert want(["--config3", "on"]) == dict(none, config3=True)
    assert want(["--sub-records", "on"]) == dict(none, config3=True, sub_records=True)
    assert want(["--full"], emu=True) == none
    assert want(["--full", "--gpus", "2"], world=2, emu=True) == dict(none, config3=True)


def test_bench_dump_outputs_caps_size(tmp_path):
    """An output above 64 MB is dumped as a fixed seeded sample of whole clips, in clip order; a smaller one whole."""
    import numpy as np
    import bench
    poses = np.repeat(np.arange(40, dtype=np.float32), 1000 * 500).reshape(40, 1000, 500)       # 2e6 bytes per clip, 8e7 in all
    bench.dump_outputs(str(tmp_path / "a"), poses)
    bench.dump_outputs(str(tmp_path / "b"), poses)
    a = np.load(str(tmp_path / "a" / "poses.npy"))
    assert a.shape == (bench.DUMP_BYTES // poses[0].nbytes, 1000, 500) and a.nbytes <= bench.DUMP_BYTES
    ids = a[:, 0, 0]
    assert (np.diff(ids) > 0).all() and all((a[i] == ids[i]).all() for i in range(len(ids)))
    assert np.array_equal(a, np.load(str(tmp_path / "b" / "poses.npy")))
    bench.dump_outputs(str(tmp_path / "c"), poses[:5])
    assert np.array_equal(np.load(str(tmp_path / "c" / "poses.npy")), poses[:5])


def test_bench_gpus8_spawns_eight_ranks_128_clips(emu_lib, tmp_path):
    """Round-4 verdict 8b: the launch shape of BASELINE config[3] itself -- `bench.py --gpus 8 --clips-per-gpu 16` creates EIGHT ranks
    (emulated library, gloo), every rank samples its 16 of the 128 tiny clips as 4 lanes x batch 4, rank 0 gathers; gathered[c] must be
    clip c: one lane of every rank (clips r, r + 8, r + 16, r + 24 for its lane 0, ...) is re-sampled by this process on one lane and
    compared bit for bit, and every other row must be finite and distinct."""
    import numpy as np
    from diffusestylegesture_amd import config as C
    from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
    from diffusestylegesture_amd.model import DSGDenoiser
    from diffusestylegesture_amd.parallel import shard_clips
    from diffusestylegesture_amd.sample import generate_clip
    from diffusestylegesture_amd.synth import synth_state_dict, synth_window_inputs
    dump = str(tmp_path / "dump")
    out = _run(["--gpus", "8", "--steps", "1", "--warmup", "0", "--precision", "fp32", "--clips-per-gpu", "16", "--dump-outputs", dump],
               {"DSG_BENCH_SKIP": "999", "DSG_EMU_THREADS": "1", "OMP_NUM_THREADS": "1"})
    assert out["n_gpus"] == 8 and out["config"]["clips_per_gpu"] == 16 and out["config"]["lanes"] == 4 and out["config"]["batch_per_lane"] == 4
    assert out["config"]["parallelism"] == "clips x8" and out["collective_backend"] == "gloo" and "5th compute queue" in out["config"]["workload"]
    got = np.load(os.path.join(dump, "poses.npy"))
    cfg = C.TINY
    assert got.shape[0] == 128 and np.isfinite(got).all()
    assert len({got[c].tobytes() for c in range(128)}) == 128          # 128 different clips
    m = DSGDenoiser(cfg, precision="fp32", max_batch=4, library=emu_lib).set_kernel_set(out["kernel_set"])
    m.load_state_dict(synth_state_dict(cfg, 20240))
    d = create_gaussian_diffusion(library=emu_lib)
    for r in range(8):
        ln = r % 4                                                      # one lane per rank, all four lane positions covered
        clips = shard_clips(128, r, 8)[ln * 4:(ln + 1) * 4]
        feats = [synth_window_inputs(cfg, 4, window=w, clips=clips)["audio"] for w in range(2)]
        want = generate_clip(m, d, feats, [1] + [0] * (cfg.style_dim_in - 1), seed=123456, smoothing=True, stream_id=clips[0], skip_timesteps=999)
        for j, c in enumerate(clips):
            assert np.array_equal(got[c], want[j]), (r, ln, c)
