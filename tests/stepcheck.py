"""TEST INFRASTRUCTURE: ONE denoising step of the fused sampler, every element against the reference's update formula at a few fp32 ulp.

Every kernel set ends a step in `gemm_epilogue_tile<EPI_OUT>` (csrc/dsg_kernels.h): guidance combination, inpainting select, clip_denoised
clamp, DDPM / DDIM update with the coefficients `build_step_tables` (csrc/dsg_hip.cpp) formed, noise lookup, zero fill of the pad columns,
store into the fp32 state and its shadow, the same once more for the unconditional twin.  The chain tests see this code through one relative
L2 norm per clip under the bf16 bound of the DENOISER (2e-2), which hides a sigma that is 10 % off.  Here the denoiser is taken out of the
comparison: `dsg_forward` and `dsg_sample` go through the same kernels and differ only in `out_mode`, so the device's own forward IS the x0
of the step (asserted bit for bit by the tests that use this helper), `dsg_noise` IS the noise of any draw, and `first_step = i`,
`max_steps = 1`, `init_noise = x_t` runs exactly loop index i.  What remains is elementwise fp32 arithmetic, in every precision mode.

The bound.  u = 2^-24 (unit roundoff of fp32), `want` = the float64 evaluation (oracle.sampler.p_step / ddim_step, dtype float64) with the
oracle's fp32-rounded coefficients.  Every element must satisfy

    |got - want|  <=  8 u S  (+ the DDIM conditioning term below),        S = the sum of the absolute values of the terms of that element
    DDPM   x = k1 x0 + k2 x_t + k3 z                      S = |k1 x0| + |k2 x_t| + |k3 z|
    DDIM   x = k3 x0 + k4 (k1 x_t - x0) / k2 + k5 z       S = |k3 x0| + |k4| E + |k5 z|,   E = (|k1 x_t| + |x0|) / k2

Derivation of the 8, term by term (first order in u; every fp32 operation rounds by at most u relative to its own result, a fused
multiply-add rounds once where the separate operations round twice, so the uncontracted evaluation is the worst case):
  DDPM.  fl(k1 x0): u |k1 x0|.  fl(k2 x_t): u |k2 x_t|.  their sum: u (|k1 x0| + |k2 x_t|).  fl(k3 z): u |k3 z|.  the last sum: u S.
         Together  <= 2u |k1 x0| + 2u |k2 x_t| + u |k3 z| + u S  <=  3 u S : five roundings, at most three on the path of one term.
         Coefficients: k1, k2 are casts of float64 tables (the same on both sides); k3 = nz expf(0.5 log variance) comes from the host C
         library on the device side and from numpy in `want`: up to 2 ulp apart, one ulp being at most 2u relative: 4u |k3 z| <= 4 u S.
         Sum 7 u S.
  DDIM.  fl(k1 x_t): u |k1 x_t|.  the difference: u (|k1 x_t| + |x0|).  the quotient: u |eps|, |eps| <= E.  So eps carries <= 3 u E.
         fl(k3 x0): u |k3 x0|.  fl(k4 eps): u k4 E.  their sum: u (|k3 x0| + k4 E).  fl(k5 z): u |k5 z|.  the last sum: u S.
         Together  <= 3u |k3 x0| + 6u k4 E + 2u |k5 z|  <=  6 u S : the longest path has six roundings, five when one pair contracts.
         Coefficients: sqrtf, the division and the products are correctly rounded on both sides, so k1 .. k3 and k5 agree unless the host
         compiler contracts a product into a sum; that can only happen in the argument of k4 = sqrt(1 - abar_prev - sigma^2), below.
  8 leaves one u (DDPM) / two u (DDIM) for the second-order terms and for a float64 table entry that rounds to the neighbouring fp32
  number.  The constant is derived, not fitted: the measured ratios are for information only.
The DDIM conditioning term.  a = 1 - abar_prev - sigma^2 is a difference of numbers of size 1, so a contracted `sigma * sigma` and a sigma
that is an ulp apart move it by up to 2u ABSOLUTE, and k4 = sqrt(a) by up to 2u / (2 k4) = u / k4 -- far more than 8 u k4 when a is small
(eta = 1: a -> 0).  The bound therefore gets  (u / k4) E  added for k4 > 0.  For k4 = 0 (schedule index 0: abar_prev = 1, sigma = 0; any
index at eta = 1 where a is 0) the argument is exactly 0 on both sides and nothing is added.

No element is left out: the comparison covers all B x J x T outputs.  The pad columns j >= J of the state cannot be read from
[B, J, 1, T]; they, the bf16 / fragment-major shadow and the twin rows are covered by running a second step on top of the first (a wrong
shadow, twin or pad column moves the second step's x0, which is then no longer the forward of the first step's output).

This module imports no GPU library: the callers hand in the model, and `device_noise` goes through the model's own library object."""
import ctypes as C

import numpy as np

from oracle import sampler

U = 2.0 ** -24
K_BOUND = 8.0
DDPM, DDIM = 0, 1          # = lib.MODE_DDPM / MODE_DDIM


def loop_to_index(n, i):
    """Schedule index of loop index i of an n-step chain (the loops run the schedule backwards)."""
    return n - 1 - i


def loop_indices(n):
    """The loop indices every case runs: the first step, one in the middle, n - 2, and n - 1 (schedule index 0: no noise, k2 = 0)."""
    return (0, n // 2 - 3, n - 2, n - 1)


def coefs(odiff, mode, idx, eta=0.0):
    """The oracle's fp32 coefficients of schedule index idx, in the order of the device's step tables (k1 .. k3 / k1 .. k5)."""
    return sampler.p_coefs(odiff, idx) if mode == DDPM else sampler.ddim_coefs(odiff, idx, eta)


def select_clamp(x0, mask=None, motion=None, clip_denoised=False):
    """gaussian_diffusion.py:317-321 then :377-379: the constraint replaces the prediction BEFORE the clamp (both exact in fp32)."""
    x0 = np.asarray(x0, np.float32)
    if mask is not None:
        x0 = np.where(np.asarray(mask) != 0, np.asarray(motion, np.float32), x0)
    if clip_denoised:
        x0 = np.clip(x0, np.float32(-1), np.float32(1))
    return x0


def step64(odiff, mode, idx, x0c, x_t, z, eta=0.0, const_noise=False):
    """(want64, (S, extra)): the float64 step on the selected + clamped x0 and the two parts of the bound of every element."""
    x0d, xtd = np.asarray(x0c, np.float32).astype(np.float64), np.asarray(x_t, np.float32).astype(np.float64)
    zd = np.asarray(z, np.float32).astype(np.float64)
    if const_noise:
        zd = np.repeat(zd[[0]], x0d.shape[0], 0)
    k = [float(c) for c in coefs(odiff, mode, idx, eta)]
    if mode == DDPM:
        want = sampler.p_step(odiff, idx, x0c, x_t, z, False, const_noise, dtype=np.float64)
        S = np.abs(k[0] * x0d) + np.abs(k[1] * xtd) + np.abs(k[2] * zd)
        extra = np.zeros_like(S)
    else:
        want = sampler.ddim_step(odiff, idx, x0c, x_t, z, eta, False, dtype=np.float64)
        E = (np.abs(k[0] * xtd) + np.abs(x0d)) / k[1]
        S = np.abs(k[2] * x0d) + abs(k[3]) * E + np.abs(k[4] * zd)
        extra = (U / k[3]) * E if k[3] > 0 else np.zeros_like(S)
    return want, (S, extra)


def device_noise(lib, shape, seed, stream_id, draw):
    """Draw `draw` of (seed, stream_id) as the library itself produces it (dsg_noise): the very noise the fused step uses."""
    out = np.zeros(shape, np.float32)
    lib.check(lib.cdll.dsg_noise(out.ctypes.data, int(shape[0]), int(shape[1]) * int(shape[2]), int(shape[3]), C.c_uint64(seed),
                                 C.c_uint64(stream_id), int(draw), None))
    return out


def _kwargs(y, scale, mask, motion):
    yy = dict(y)
    if scale is not None:
        yy["scale"] = np.asarray(scale, np.float32)
    if mask is not None:
        yy["inpainting_mask"], yy["inpainted_motion"] = mask, motion
    return {"y": yy}


def one_step(model, diffusion, mode, i, x_t, y, *, scale=None, mask=None, motion=None, clip_denoised=False, const_noise=False, eta=0.0,
             step_noise=None, seed=0, stream_id=0, draw_base=0, n_steps=1):
    """Loop index i alone (or n_steps steps from i on) through DSGDiffusion._fused: first_step = i, max_steps = n_steps, init_noise = x_t,
    skip_timesteps = 0.  `model` is the DSGDenoiser; `scale` [B] switches fused guidance on (max_batch >= 2 B).  Returns x_{t-1} as numpy."""
    shape = tuple(np.asarray(x_t).shape)
    diffusion.manual_seed(seed, stream_id)
    out = diffusion._fused(mode, model, scale is not None, shape, x_t, _kwargs(y, scale, mask, motion), 0, None, None, const_noise, eta,
                           step_noise, seed, draw_base, clip_denoised, first_step=i, max_steps=n_steps)
    return np.asarray(out)


def lanes_one_step(models, diffusion, mode, i, x_ts, ys, *, seeds, stream_ids, draw_base=0, eta=0.0, clip_denoised=False):
    """`one_step` for several lanes at once through dsg_sample_multi (the argument blocks are DSGDiffusion._prepare's)."""
    n = len(models)
    lib = models[0].lib
    shape = tuple(np.asarray(x_ts[0]).shape)
    from diffusestylegesture_amd import lib as L
    args = (L.dsg_sample_args * n)()
    keeps, outs = [], []
    for k, m in enumerate(models):
        a, keep, _, _ = diffusion._prepare(mode, m, False, shape, x_ts[k], {"y": ys[k]}, 0, None, None, False, eta, None, seeds[k], draw_base,
                                           clip_denoised, stream_id=stream_ids[k], first_step=i, max_steps=1)
        args[k] = a
        keeps.append(keep)
        outs.append(np.empty(shape, np.float32))
    hs = (C.c_void_p * n)(*[m.handle for m in models])
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    lib.check(lib.cdll.dsg_sample_multi(hs, n, args, optrs, int(shape[0]), None))
    return outs


def expected(model, odiff, mode, i, x_t, y, *, scale=None, mask=None, motion=None, clip_denoised=False, const_noise=False, eta=0.0,
             step_noise=None, seed=0, stream_id=0, draw_base=0, x0=None):
    """(want64, terms, x0) of loop index i: x0 = the device's own forward at timestep_map[n - 1 - i] (pass `x0` to reuse one), the select, the
    clamp, z = dsg_noise at draw draw_base + 1 + i (under const_noise clip 0's for everyone) or step_noise[i], then the float64 step."""
    n = odiff.num_timesteps
    idx = loop_to_index(n, i)
    x_t = np.asarray(x_t, np.float32)
    B = x_t.shape[0]
    if x0 is None:
        ts = np.full((B,), odiff.timestep_map[idx], np.int64)
        x0 = np.asarray(model.forward(x_t, ts, dict(y), cfg_scale=None if scale is None else np.asarray(scale, np.float32)))
    x0c = select_clamp(x0, mask, motion, clip_denoised)
    if step_noise is not None:
        z = np.asarray(step_noise, np.float32)         # the slice of loop index i, [B, J, 1, T]
    else:
        z = device_noise(model.lib, x_t.shape, seed, stream_id, draw_base + 1 + i)
    want, terms = step64(odiff, mode, idx, x0c, x_t, z, eta, const_noise)
    return want, terms, x0


def ratios(got, want64, terms):
    """|got - want| / bound per element (0 where both are 0, inf where the bound is 0 and the error is not, or `got` is not finite)."""
    S, extra = terms
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want64.shape == S.shape, (got.dtype, got.shape, want64.shape, S.shape)
    err = np.abs(got.astype(np.float64) - want64)
    bound = K_BOUND * U * S + extra
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got), r, np.inf)


def assert_step_exact(got, want64, terms, tag=""):
    """Every element of `got` [B, J, 1, T] within 8 u S (+ the DDIM term) of `want64`; none is excluded.  Returns the largest ratio to the
    bound.  A failure names the ten worst elements: clip, frame, feature, the 16-row tile of the element's token row b (T + 1) + f + 1 in
    the encoder's row buffer, ratio -- as tests/rowcheck.py does for rows."""
    assert np.isfinite(want64).all(), f"{tag}: the reference step is not finite"
    r = ratios(got, want64, terms)
    B, J, _, T = r.shape
    assert r.size == B * J * T                       # no element is left out
    worst = float(r.max())
    if not worst <= 1.0:
        bad = r > 1.0
        order = np.argsort(-r.reshape(-1), kind="stable")[:10]
        items = []
        for b, j, _, f in zip(*np.unravel_index(order, r.shape)):
            tok = int(b) * (T + 1) + int(f) + 1
            items.append(f"(clip {b}, frame {f}, feature {j}, tile {tok // 16}, {r[b, j, 0, f]:.3g})")
        raise AssertionError(f"{tag}: {int(bad.sum())} of {r.size} elements beyond 8 u S; clips {sorted(set(int(b) for b in np.argwhere(bad)[:, 0]))[:24]}; "
                             f"worst: " + ", ".join(items))
    return worst


# ---- the case structure shared by tests/test_emu_step_exact.py and tests/test_gpu_step_exact.py ----------------------------------------
# (name, sampler, schedule, arguments): "ddpm" schedule = 1000 steps, "ddim50" = respaced to 50.  `ext`: step_noise instead of the Philox stream.
# step_noise is [n_steps, B, J, 1, T] for the WHOLE chain (indexed by the absolute step), 19 GB for 48 ZEGGS clips at 1000 steps: the DDPM update
# with replayed noise therefore runs on the 50-step schedule in every case ("ddpm50-ext": the same epilogue branch, the same index arithmetic)
# and on the 1000-step schedule where the buffer stays under EXT_CAP_BYTES.
EXT_CAP_BYTES = 2 << 30
MODES = (("ddpm", DDPM, "ddpm", {}),
         ("ddpm-clip", DDPM, "ddpm", {"clip_denoised": True}),
         ("ddpm-const", DDPM, "ddpm", {"const_noise": True}),
         ("ddpm-ext", DDPM, "ddpm", {"ext": True}),
         ("ddpm50-ext", DDPM, "ddim50", {"ext": True}),
         ("ddim-eta0", DDIM, "ddim50", {"eta": 0.0}),
         ("ddim-eta0.5", DDIM, "ddim50", {"eta": 0.5}),
         ("ddim-eta1", DDIM, "ddim50", {"eta": 1.0}),
         ("ddim-eta0.5-clip", DDIM, "ddim50", {"eta": 0.5, "clip_denoised": True}),
         ("ddim-eta1-ext", DDIM, "ddim50", {"eta": 1.0, "ext": True}))
X_AMP = 1.0


def numpy_ext(n, shape, i, z):
    """step_noise of an n-step chain with only slice i filled (host memory; the library copies the whole chain)."""
    buf = np.zeros((n,) + tuple(shape), np.float32)
    buf[i] = z
    return buf


class Case:
    """One (dims, precision, kernel set, batch[, guidance, inpainting]) of the case tables: the model, its two schedules (library side and
    oracle side), the inputs, and a cache of the device's forwards (one per schedule and loop index, shared by all modes)."""

    def __init__(self, model, kset, B, y, scale=None, mask=None, motion=None, ext=numpy_ext, tag=""):
        from diffusestylegesture_amd.diffusion import create_gaussian_diffusion
        from oracle.schedule import OracleDiffusion
        self.model, self.kset, self.B, self.y, self.scale, self.mask, self.motion, self.ext, self.tag = model, kset, B, y, scale, mask, motion, ext, tag
        self.shape = (B, model.cfg.njoints, 1, model.cfg.n_poses)
        self.diff = {"ddpm": create_gaussian_diffusion(library=model.lib), "ddim50": create_gaussian_diffusion("ddim50", library=model.lib)}
        self.odiff = {"ddpm": OracleDiffusion(), "ddim50": OracleDiffusion(timestep_respacing="ddim50")}
        self._fwd = {}

    def x_t(self, sched, i):
        r = np.random.RandomState(7000 + 13 * i + (0 if sched == "ddpm" else 1))
        return (X_AMP * r.randn(*self.shape)).astype(np.float32)

    def forward(self, sched, i, x_t=None):
        """The device's x0 of loop index i (guidance included, no constraint, no clamp: dsg_forward does neither)."""
        key = (sched, i)
        if x_t is not None or key not in self._fwd:
            od = self.odiff[sched]
            ts = np.full((self.B,), od.timestep_map[loop_to_index(od.num_timesteps, i)], np.int64)
            x0 = np.asarray(self.model.forward(self.x_t(sched, i) if x_t is None else x_t, ts, dict(self.y), cfg_scale=self.scale))
            assert self.model.last_kernel_set() == self.kset, (self.tag, self.model.last_kernel_set())
            if x_t is not None:
                return x0
            x0.setflags(write=False)
            self._fwd[key] = x0
        return self._fwd[key]

    def step(self, mode, sched, i, x_t, n_steps=1, constrained=True, **kw):
        kw = dict(kw)
        kw.pop("ext", None)
        m = (self.mask, self.motion) if constrained else (None, None)
        out = one_step(self.model, self.diff[sched], mode, i, x_t, self.y, scale=self.scale, mask=m[0], motion=m[1], n_steps=n_steps, **kw)
        assert self.model.last_kernel_set() == self.kset, (self.tag, self.model.last_kernel_set())
        return out

    def check(self, name, mode, sched, i, args, seed=5, stream_id=2, draw_base=0, x_t=None, x0=None):
        """Test B for one (mode, loop index): the step on the device, every element of every clip against the float64 step."""
        od = self.odiff[sched]
        n = od.num_timesteps
        if x_t is None:
            x_t, x0 = self.x_t(sched, i), self.forward(sched, i)
        kw = {k: v for k, v in args.items() if k != "ext"}
        z = sn = None
        if args.get("ext"):
            z = np.random.RandomState(900 + i).randn(*self.shape).astype(np.float32)
            sn = self.ext(n, self.shape, i, z)
        got = self.step(mode, sched, i, x_t, step_noise=sn, seed=seed, stream_id=stream_id, draw_base=draw_base, **kw)
        want, terms, _ = expected(self.model, od, mode, i, x_t, self.y, scale=self.scale, mask=self.mask, motion=self.motion, step_noise=z,
                                  seed=seed, stream_id=stream_id, draw_base=draw_base, x0=x0, **kw)
        if kw.get("clip_denoised"):
            x0s = select_clamp(x0, self.mask, self.motion)
            frac = float(np.mean(np.abs(x0s) > 1))
            assert 0 < frac < 1, f"{self.tag} {name} i={i}: the clamp case needs part of x0 beyond +-1, has {frac:.3f}"
        return assert_step_exact(got, want, terms, f"{self.tag} {name} i={i}")

    def modes(self):
        nbytes = lambda sched: 4 * self.odiff[sched].num_timesteps * int(np.prod(self.shape))
        return [m for m in MODES if not (m[3].get("ext") and nbytes(m[2]) > EXT_CAP_BYTES)]

    def check_all(self, indices=None, modes=None):
        """Test B: every mode x loop index; returns {mode name: worst ratio to the bound}."""
        worst = {}
        for name, mode, sched, args in (self.modes() if modes is None else modes):
            n = self.odiff[sched].num_timesteps
            for i in (loop_indices(n) if indices is None else indices(n)):
                worst[name] = max(worst.get(name, 0.0), self.check(name, mode, sched, i, args))
        return worst

    def check_last_step_is_forward(self):
        """Test A: the last DDPM step (k1 = 1, k2 = 0, no noise; no constraint, no clamp) returns forward(x_t, timestep_map[0]) bit for bit."""
        d = self.diff["ddpm"]
        n = d.num_timesteps
        assert np.float32(d.posterior_mean_coef1[0]) == np.float32(1.0) and np.float32(d.posterior_mean_coef2[0]) == 0.0
        assert d.timestep_map[0] == self.odiff["ddpm"].timestep_map[0]
        got = self.step(DDPM, "ddpm", n - 1, self.x_t("ddpm", n - 1), constrained=False, seed=5, stream_id=2)
        x0 = self.forward("ddpm", n - 1)
        diff = got != x0
        assert not diff.any(), (f"{self.tag}: the last DDPM step is not the forward in {int(diff.sum())} of {diff.size} elements, clips "
                                f"{sorted(set(int(b) for b in np.argwhere(diff)[:, 0]))[:24]}, max |d| {np.abs(got - x0).max():.3e}")

    def check_two_steps(self, name, mode, sched, args, i=None):
        """Test C: two steps in one call == two one-step calls, bit for bit, and the second step passes B with x0 = forward(out_1): a wrong
        bf16 / fragment-major shadow, wrong twin rows or a non-zero pad column of the state would move the second step's x0."""
        n = self.odiff[sched].num_timesteps
        i = loop_indices(n)[1] if i is None else i
        x_t = self.x_t(sched, i)
        kw = dict(args, seed=5, stream_id=2, draw_base=3)
        both = self.step(mode, sched, i, x_t, n_steps=2, **kw)
        out1 = self.step(mode, sched, i, x_t, **kw)
        out2 = self.step(mode, sched, i + 1, out1, **kw)
        assert np.array_equal(both, out2), f"{self.tag} {name}: two steps in one call differ from two calls in {int((both != out2).sum())} elements"
        x0 = self.forward(sched, i + 1, x_t=out1)
        want, terms, _ = expected(self.model, self.odiff[sched], mode, i + 1, out1, self.y, scale=self.scale, mask=self.mask, motion=self.motion,
                                  x0=x0, **kw)
        return assert_step_exact(both, want, terms, f"{self.tag} {name} second of two steps from i={i}")
