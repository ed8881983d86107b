"""CPU, no library: the check of tests/stepcheck.py itself.  The "model" is a fixed random x0, `got` is the fp32 oracle step
(oracle.sampler.p_step / ddim_step, the loops' own arithmetic), `want` the float64 step.  First the reference alone must stay within the
bound 8 u S on every input of the case lists of the emulator / GPU files (every loop index, mode, eta and clamp setting; tiny and ZEGGS
shapes); then each of ten ways a fused epilogue or its step tables can be subtly wrong must FAIL the check, and be named."""
import numpy as np
import pytest

from oracle import philox, sampler
from oracle.schedule import OracleDiffusion
from tests import stepcheck as S

SHAPES = {"tiny": (5, 37, 1, 22), "zeggs": (3, 1141, 1, 88)}
_OD = {}


def odiff(mode):
    if mode not in _OD:
        _OD[mode] = OracleDiffusion() if mode == S.DDPM else OracleDiffusion(timestep_respacing="ddim50")
    return _OD[mode]


def inputs(shape, i, amp=1.0, seed=0):
    """(x0, x_t, z): a fixed random x0 in place of a model (part of it beyond +-1, so the clamp acts), x_t, and draw 1 + i of the noise stream."""
    r = np.random.RandomState(1000 * seed + i)
    x0 = (0.9 * amp * r.randn(*shape)).astype(np.float32)
    x_t = (amp * r.randn(*shape)).astype(np.float32)
    return x0, x_t, philox.normal_bj1t(shape, 11 + seed, 1 + i, 3)


def f32_step(mode, k, x0c, x_t, z):
    """The update in fp32 with explicit coefficients k, in the oracle's evaluation order: the form the mutations below are applied to."""
    k = [np.float32(c) for c in k]
    if mode == S.DDPM:
        return (k[0] * x0c + k[1] * x_t) + k[2] * z
    eps = (k[0] * x_t - x0c) / k[1]
    return ((x0c * k[2] + k[3] * eps) + k[4] * z).astype(np.float32)


def got_want(mode, i, shape, eta=0.0, clip=False, const_noise=False, mask=None, motion=None):
    od = odiff(mode)
    idx = S.loop_to_index(od.num_timesteps, i)
    x0, x_t, z = inputs(shape, i)
    x0c = S.select_clamp(x0, mask, motion, clip)
    want, terms = S.step64(od, mode, idx, x0c, x_t, z, eta, const_noise)
    if mode == S.DDPM:
        got = sampler.p_step(od, idx, x0c, x_t, z, False, const_noise)
    else:
        got = sampler.ddim_step(od, idx, x0c, x_t, z, eta, False)
    return dict(od=od, idx=idx, x0=x0, x0c=x0c, x_t=x_t, z=z, want=want, terms=terms, got=got, k=S.coefs(od, mode, idx, eta))


def test_the_reference_alone_is_within_the_bound_on_every_input():
    worst = {}
    for name, shape in SHAPES.items():
        for mode, etas in ((S.DDPM, (0.0,)), (S.DDIM, (0.0, 0.5, 1.0))):
            n = odiff(mode).num_timesteps
            for i in S.loop_indices(n):
                for eta in etas:
                    for clip in (False, True):
                        for const_noise in ((False, True) if mode == S.DDPM else (False,)):
                            c = got_want(mode, i, shape, eta, clip, const_noise)
                            assert c["got"].dtype == np.float32
                            if clip:
                                frac = float(np.mean(np.abs(c["x0"]) > 1))
                                assert 0.05 < frac < 0.95 and np.abs(c["x0c"]).max() == 1.0
                            tag = f"{name} {'ddpm' if mode == S.DDPM else 'ddim'} i={i} eta={eta} clip={clip} const={const_noise}"
                            w = S.assert_step_exact(c["got"], c["want"], c["terms"], tag)
                            worst[name, mode] = max(worst.get((name, mode), 0.0), w)
    for (name, mode), w in sorted(worst.items()):
        print(f"STEPCHECK reference alone, {name} {'ddpm' if mode == S.DDPM else 'ddim'}: worst element at {w:.3f} x the bound")
    assert max(worst.values()) <= 1.0


def test_the_fp32_step_functions_are_what_f32_step_restates():
    """The mutations below are applied to `f32_step`; unmutated it is the oracle's fp32 step bit for bit, and k1 == 1, k2 == 0, k3 == 0 at the last DDPM step."""
    for mode, eta in ((S.DDPM, 0.0), (S.DDIM, 0.5)):
        for i in S.loop_indices(odiff(mode).num_timesteps):
            c = got_want(mode, i, SHAPES["tiny"], eta)
            assert np.array_equal(f32_step(mode, c["k"], c["x0c"], c["x_t"], c["z"]), c["got"])
    k = S.coefs(odiff(S.DDPM), S.DDPM, 0)
    assert k[0] == np.float32(1.0) and k[1] == 0 and k[2] == 0


def _must_fail(got, c, what):
    with pytest.raises(AssertionError) as e:
        S.assert_step_exact(got, c["want"], c["terms"], what)
    msg = str(e.value)
    assert what in msg and "elements beyond 8 u S" in msg and "(clip " in msg and "feature" in msg and "tile" in msg, msg
    return msg


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_listed_mutation_fails_and_is_named(name):
    shape = SHAPES[name]
    B = shape[0]
    nP, nD = odiff(S.DDPM).num_timesteps, odiff(S.DDIM).num_timesteps
    mid = S.loop_indices(nP)[1]
    # noise kept at schedule index 0 (nz): DDPM, the last step.  (DDIM has sigma = 0 there with or without nz: abar_prev = 1.)
    c = got_want(S.DDPM, nP - 1, shape)
    k3 = np.exp(np.float32(0.5) * np.float32(c["od"].t["posterior_log_variance_clipped"][0]))
    _must_fail(f32_step(S.DDPM, (c["k"][0], c["k"][1], k3), c["x0c"], c["x_t"], c["z"]), c, "noise kept at index 0")
    # the coefficients of index i + 1 / i - 1
    for mode, eta, n in ((S.DDPM, 0.0, nP), (S.DDIM, 0.5, nD)):
        for i in (S.loop_indices(n)[1], n - 2):
            c = got_want(mode, i, shape, eta)
            for d in (1, -1):
                _must_fail(f32_step(mode, S.coefs(c["od"], mode, c["idx"] + d, eta), c["x0c"], c["x_t"], c["z"]), c, f"coefficients of index i{d:+d}")
    # sigma x 1.05
    c = got_want(S.DDPM, mid, shape)
    _must_fail(f32_step(S.DDPM, (c["k"][0], c["k"][1], np.float32(1.05) * c["k"][2]), c["x0c"], c["x_t"], c["z"]), c, "sigma x 1.05 (ddpm)")
    c = got_want(S.DDIM, S.loop_indices(nD)[1], shape, 0.5)
    t = c["od"].t
    sig = np.float32(1.05) * c["k"][4]
    k4 = np.sqrt(np.float32(1) - np.float32(t["alphas_cumprod_prev"][c["idx"]]) - sig * sig)
    _must_fail(f32_step(S.DDIM, c["k"][:3] + (k4, sig), c["x0c"], c["x_t"], c["z"]), c, "sigma x 1.05 (ddim)")
    # the clamp applied after the update instead of before it
    c = got_want(S.DDPM, mid, shape, clip=True)
    _must_fail(np.clip(f32_step(S.DDPM, c["k"], c["x0"], c["x_t"], c["z"]), np.float32(-1), np.float32(1)), c, "clamp after the update")
    # the select applied after the clamp (the motion has values beyond +-1)
    r = np.random.RandomState(5)
    mask = np.zeros(shape, bool)
    mask[:, :shape[1] // 2] = True
    motion = (1.5 * r.randn(*shape)).astype(np.float32)
    c = got_want(S.DDPM, mid, shape, clip=True, mask=mask, motion=motion)
    wrong = np.where(mask, motion, np.clip(c["x0"], np.float32(-1), np.float32(1)))
    _must_fail(f32_step(S.DDPM, c["k"], wrong, c["x_t"], c["z"]), c, "select after the clamp")
    # clip b's noise taken from clip b - 1
    c = got_want(S.DDPM, mid, shape)
    _must_fail(f32_step(S.DDPM, c["k"], c["x0c"], c["x_t"], np.roll(c["z"], 1, 0)), c, "noise of clip b - 1")
    # the noise of one feature quad shifted by one quad
    z = c["z"].copy()
    z[:, 4:8] = c["z"][:, 8:12]
    msg = _must_fail(f32_step(S.DDPM, c["k"], c["x0c"], c["x_t"], z), c, "one noise quad shifted")
    assert int(msg.split(": ")[1].split(" of")[0]) <= B * 4 * shape[3]          # nothing outside the quad is flagged
    # const_noise ignored
    c = got_want(S.DDPM, mid, shape, const_noise=True)
    msg = _must_fail(f32_step(S.DDPM, c["k"], c["x0c"], c["x_t"], c["z"]), c, "const_noise ignored")
    assert "clips [1" in msg                     # clip 0 has its own noise either way
    # eta ignored
    c = got_want(S.DDIM, S.loop_indices(nD)[1], shape, 0.5)
    _must_fail(f32_step(S.DDIM, S.coefs(c["od"], S.DDIM, c["idx"], 0.0), c["x0c"], c["x_t"], c["z"]), c, "eta ignored")
    # one element 32 ulp off: the element that cancels least (32 ulp >= 32 u |x|, the bound is 8 u S with S >= |x|)
    for mode, eta, n in ((S.DDPM, 0.0, nP), (S.DDIM, 0.5, nD)):
        c = got_want(mode, S.loop_indices(n)[1], shape, eta)
        Sb, extra = c["terms"]
        at = np.unravel_index(np.argmax(np.abs(c["want"]) / (S.K_BOUND * S.U * Sb + extra)), shape)
        got = c["got"].copy()
        got.view(np.int32)[at] += 32
        msg = _must_fail(got, c, "one element 32 ulp off")
        assert msg.split(": ")[1].startswith("1 of") and f"(clip {at[0]}, frame {at[3]}, feature {at[1]}, tile {(at[0] * (shape[3] + 1) + at[3] + 1) // 16}," in msg
