"""Host-side mirror of the reference sampler interface, backed by the HIP library.

Reference interface mirrored (same names, argument order, defaults and error behaviour):
  * `get_named_beta_schedule`, `betas_for_alpha_bar`          main/diffusion/gaussian_diffusion.py:21-65
  * `space_timesteps`, `SpacedDiffusion`                       main/diffusion/respace.py:8-114
  * `GaussianDiffusion.p_sample_loop` / `ddim_sample_loop`     main/diffusion/gaussian_diffusion.py:608-671, :889-936
  * `q_sample`, `_predict_xstart_from_eps`, `q_posterior_mean_variance`, `p_sample`, `ddim_sample`
                                                               :236-278, :400-405, :506-558, :742-792
  * `create_gaussian_diffusion()`                              main/utils/model_util.py:59-100
The whole step loop of `p_sample_loop(model=DSGDenoiser, ...)` runs inside libdsg_hip.so (one hipGraph replay per
`steps_per_graph` steps, no host involvement per step).  Handing any other callable as `model` runs the generic
loop: the callable produces x0 and the fused HIP elementwise kernels (dsg_posterior_step / dsg_ddim_step /
dsg_q_sample) do the sampler arithmetic on the device tensors.

Noise: the reference consumes torch's global generator.  Here every draw comes from the framework's counter-based
stream (Philox4x32-10, see csrc/dsg_kernels.h) addressed by (seed, stream_id, draw index).  `manual_seed(seed)`
plays the role of `torch.manual_seed(seed)` (sample.py:212): it resets the draw counter, and each sampling call
advances it by 1 + n_steps, so consecutive windows of a clip continue one stream exactly like the reference does.
`clip_streams=` (every loop): one Philox stream PER BATCH ELEMENT -- element b draws what it would draw sampled alone (batch 1)
after `manual_seed(seed_b, stream_b)`, so a clip's result does not depend on the batch, slot, lane or rank it rides in.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import lib as L


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    n = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)],
                    dtype=np.float64)


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps, scale_betas=1.):
    if schedule_name == "linear":
        scale = scale_betas * 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps,
                                   lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def space_timesteps(num_timesteps, section_counts):
    """Kept-step set; "ddimN" = the DDIM paper's fixed stride, "a,b,c" = per-section counts."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            desired = int(section_counts[len("ddim"):])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == desired:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    per, extra = divmod(num_timesteps, len(section_counts))
    steps, start = [], 0
    for i, count in enumerate(section_counts):
        size = per + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        pos = 0.0
        for _ in range(count):
            steps.append(start + round(pos))
            pos += stride
        start += size
    return set(steps)


_TABLES = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
           "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
           "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


_U64 = 2 ** 64 - 1


def _clip_streams(clip_streams, B, what="clip_streams"):
    """`clip_streams=` as (seeds or None, stream ids): a sequence of B stream ids (every element keeps the call's seed), or of B
    (seed, stream_id) pairs."""
    cs = list(clip_streams)
    if len(cs) != B:
        raise ValueError(f"{what}: {len(cs)} entries for a batch of {B}")
    pairs = [isinstance(c, (tuple, list)) for c in cs]
    if any(pairs):
        if not all(pairs) or any(len(c) != 2 for c in cs):
            raise ValueError(f"{what}: B stream ids, or B (seed, stream_id) pairs")
        return [int(c[0]) & _U64 for c in cs], [int(c[1]) & _U64 for c in cs]
    return None, [int(c) & _U64 for c in cs]


class _keyed:
    """The lanes' per-element noise streams for ONE call (`DSGDenoiser.set_noise_streams`): set on entry, cleared on exit, as the
    clip-level constraint of `sample_clip` is.  `per_lane`: one `clip_streams` (or None) per lane."""

    def __init__(self, lanes, per_lane, B):
        self.lanes, self.streams = list(lanes), [None if cs is None else _clip_streams(cs, B) for cs in per_lane]

    def __enter__(self):
        for m, st in zip(self.lanes, self.streams):
            if st is not None:
                m.set_noise_streams(*st)
            elif m.noise_streams:
                m.set_noise_streams(None, None)
        return self

    def __exit__(self, *exc):
        for m in self.lanes:
            if m.noise_streams:
                m.set_noise_streams(None, None)
        return False


def _inner_lanes(lanes, who, batch=None):
    """The lanes of a multi-lane / clip / queue call -- a model or a list of them -- as (their DSGDenoisers, their guided flags):
    `_library_model` per lane; a lane that is no library model is the TypeError of `who`."""
    lanes = list(lanes) if isinstance(lanes, (list, tuple)) else [lanes]
    pairs = [DSGDiffusion._library_model(m, batch) for m in lanes]
    if any(inner is None for inner, _ in pairs):
        raise TypeError(f"{who} drives library denoisers (DSGDenoiser lanes)")
    return [inner for inner, _ in pairs], [guided for _, guided in pairs]


def _queue_mask(mask_local, T, who):
    """`mask_local=` of the queue entry points as a Buf: one mask of T entries shared by every slot ("ones": all of them set)"""
    mbuf = L.Buf(np.ones((T,), np.uint8) if isinstance(mask_local, str) else mask_local, "uint8")
    if mbuf.obj is not None and int(np.prod(mbuf.obj.shape)) != T:
        raise ValueError(f"{who}: mask_local is one mask of {T} entries, shared by every slot")
    return mbuf


class DSGDiffusion:
    """SpacedDiffusion(use_timesteps, betas=...) for START_X / FIXED_SMALL models (the only configuration
    `create_gaussian_diffusion` builds).  Table attributes carry the reference's names."""

    def __init__(self, use_timesteps, betas, library: L.DSGLibrary | None = None):
        base = np.array(betas, dtype=np.float64)
        if base.ndim != 1:
            raise ValueError("betas must be 1-D")
        if not ((base > 0).all() and (base <= 1).all()):
            raise ValueError("betas must be in (0, 1]")
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(base)
        ac = np.cumprod(1.0 - base)
        last, nb, tmap = 1.0, [], []
        for i, a in enumerate(ac):
            if i in self.use_timesteps:
                nb.append(1 - a / last)
                last = a
                tmap.append(i)
        self.timestep_map = tmap
        self.num_timesteps = len(nb)
        self._lib = library
        self._set_tables(np.array(nb, dtype=np.float64))
        self.rescale_timesteps = False
        self._seed, self._draw, self.stream_id = 0, 0, 0
        self.last_sample_ms = None

    # the tables are computed by the library's own host code (dsg_schedule_tables), the same code dsg_set_schedule
    # uses on the device path -- so the CPU tests pin exactly what the sampler consumes
    def _set_tables(self, betas):
        n = len(betas)
        lib = self._lib or L.default_library()
        self._lib = lib
        out = np.zeros((11, n), dtype=np.float64)
        lib.check(lib.cdll.dsg_schedule_tables(betas.ctypes.data, n, out.ctypes.data))
        for i, k in enumerate(_TABLES):
            setattr(self, k, out[i].copy())

    # ---- RNG stream ------------------------------------------------------------------------------------------
    def manual_seed(self, seed: int, stream_id: int = 0):
        self._seed, self._draw, self.stream_id = int(seed), 0, int(stream_id)
        return self

    # ---- fused loops -----------------------------------------------------------------------------------------
    def _check_unsupported(self, denoised_fn, cond_fn, randomize_class, cond_fn_with_grad):
        """Sampler hooks (gaussian_diffusion.py:364-370, :428-441, :458-480).  `denoised_fn` and `cond_fn` are Python callables evaluated once
        per step: a loop that carries one runs step by step in the generic loop (the denoiser through the library, the hook in torch, the update
        kernels of the library) instead of as one fence-free chain inside the library -- returns True then.  `cond_fn_with_grad` needs autograd
        through the denoiser and `randomize_class` a class-conditional model (`model.num_classes`: the MDM denoisers of this path have none,
        the reference raises AttributeError there): both stay NotImplementedError."""
        if randomize_class or cond_fn_with_grad:
            raise NotImplementedError("randomize_class / cond_fn_with_grad are not supported")
        return denoised_fn is not None or cond_fn is not None

    @staticmethod
    def _library_model(model, batch=None):
        """(denoiser, guided) when the whole step loop can run inside the library: a DSGDenoiser, or the classifier-free
        guidance wrapper around one WITH ROOM for the unconditional twins (max_batch >= 2 * batch).  A wrapper around a
        smaller denoiser is not a library model: the generic loop takes it (two library calls per step, the same Philox
        stream), as it did before guidance was fused."""
        from .model import ClassifierFreeSampleModel, DSGDenoiser
        if isinstance(model, DSGDenoiser):
            return model, False
        if isinstance(model, ClassifierFreeSampleModel) and isinstance(model.model, DSGDenoiser):
            if batch is not None and model.model.max_batch < 2 * int(batch):
                return None, False
            return model.model, True
        return None, False

    def _clip_args(self, ddim, eta, skip_timesteps, clip_denoised, seed=None, stream_id=0):
        """the dsg_sample_args of a clip or queue call: the sampler, and the stream (`seed`, default the one of `manual_seed`; `stream_id`)
        at this object's draw counter"""
        a = L.dsg_sample_args()
        a.mode, a.skip_timesteps, a.eta = (L.MODE_DDIM if ddim else L.MODE_DDPM), int(skip_timesteps), float(eta)
        a.seed, a.stream_id, a.draw_base = int(self._seed if seed is None else seed) & _U64, int(stream_id), self._draw
        a.clip_denoised = int(bool(clip_denoised))
        return a

    def _prepare(self, mode, model, guided, shape, noise, model_kwargs, skip_timesteps, init_image, dump_steps,
                 const_noise, eta, step_noise, seed, draw_base, clip_denoised, stream_id=None, first_step=0, max_steps=0):
        """Conditioning + schedule to the library and the argument block of one dsg_sample call."""
        B = int(shape[0])
        if tuple(shape) != (B, model.njoints, model.nfeats, model.cfg.n_poses):
            raise ValueError(f"shape {tuple(shape)} does not match the denoiser ({model.njoints}, {model.nfeats}, "
                             f"{model.cfg.n_poses})")
        y = (model_kwargs or {}).get("y")
        if y is None:
            raise ValueError("model_kwargs['y'] is required")
        model.set_schedule(self)
        # gaussian_diffusion.py:317-321: the constraint applies when BOTH keys are there (one alone is ignored, as in the reference); the
        # lane keeps it until a call without the keys switches it off -- no library call for that on a lane that never had one
        if _INPAINT_KEYS[0] in y and _INPAINT_KEYS[1] in y:
            model.set_inpainting(_inpaint_mask(y[_INPAINT_KEYS[0]]), y[_INPAINT_KEYS[1]], B)
        elif model.inpainting:
            model.set_inpainting(None, None, 0)
        y = {k: v for k, v in y.items() if k not in _INPAINT_KEYS}
        if guided:
            if "scale" not in y:
                raise KeyError("scale")
            if model.max_batch < 2 * B:
                raise ValueError("classifier-free guidance runs the unconditional twins in the same batch: create the "
                                 f"DSGDenoiser with max_batch >= {2 * B}")
            model.set_cond({k: v for k, v in y.items() if k != "scale"}, B, cfg_scale=y["scale"])
        else:
            model.set_cond(y, B)
        use_torch = any(L.is_torch(v) for v in (noise, init_image, y.get("audio")))
        keep = (L.Buf(noise), L.Buf(init_image), L.Buf(step_noise))
        a = L.dsg_sample_args()
        a.mode, a.skip_timesteps, a.eta, a.const_noise = mode, int(skip_timesteps), float(eta), int(bool(const_noise))
        a.init_noise, a.step_noise, a.init_image = keep[0].ptr, keep[2].ptr, keep[1].ptr
        a.seed = (self._seed if seed is None else int(seed)) & (2 ** 64 - 1)
        a.stream_id = self.stream_id if stream_id is None else int(stream_id)
        a.draw_base = self._draw if draw_base is None else int(draw_base)
        a.clip_denoised = int(bool(clip_denoised))
        a.first_step, a.max_steps = int(first_step), int(max_steps)
        dump = None
        if dump_steps is not None:
            ds = np.ascontiguousarray(sorted(int(d) for d in dump_steps), dtype=np.int32)
            dump = np.zeros((len(ds),) + tuple(shape), dtype=np.float32)
            a.n_dump, a.dump_steps, a.dump_out = len(ds), ds.ctypes.data, dump.ctypes.data
            keep = keep + (ds,)
        return a, keep, dump, use_torch

    def _fused(self, mode, model, guided, shape, noise, model_kwargs, skip_timesteps, init_image, dump_steps, const_noise,
               eta, step_noise, seed, draw_base, clip_denoised, first_step=0, max_steps=0, stream_id=None, clip_streams=None):
        B = int(shape[0])
        a, keep, dump, use_torch = self._prepare(mode, model, guided, shape, noise, model_kwargs, skip_timesteps, init_image,
                                                 dump_steps, const_noise, eta, step_noise, seed, draw_base, clip_denoised,
                                                 stream_id=stream_id, first_step=first_step, max_steps=max_steps)
        n_run = self.num_timesteps - skip_timesteps
        out, out_ptr = model._alloc_out(shape, use_torch)
        lib = model.lib
        with _keyed([model], [clip_streams], B):
            lib.check(lib.cdll.dsg_sample(model.handle, C.byref(a), out_ptr, B, L.current_stream_ptr() if use_torch else None))
        if draw_base is None:
            self._draw += 1 + n_run
        self._last_model = model
        if dump_steps is not None:
            lib.check(lib.cdll.dsg_sync(model.handle))
            res = [dump[i] for i in range(len(dump))]
            if use_torch:
                import torch
                res = [torch.from_numpy(d).to(out.device) for d in res]
            return res
        return out

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                      randomize_class=False, cond_fn_with_grad=False, dump_steps=None, const_noise=False,
                      *, step_noise=None, seed=None, draw_base=None, clip_streams=None):
        """`clip_streams` (every loop of this class): B stream ids, or B (seed, stream_id) pairs -- element b then draws from ITS
        Philox stream and is, bit for bit, the batch-1 call after `manual_seed(seed_b, stream_b)` with its conditioning under the same
        kernel set (`DSGDenoiser.set_noise_streams`; applied for this call, cleared after it)."""
        hooks = self._check_unsupported(denoised_fn, cond_fn, randomize_class, cond_fn_with_grad)
        inner, guided = (None, False) if hooks else self._library_model(model, shape[0])
        if inner is not None:
            return self._fused(L.MODE_DDPM, inner, guided, shape, noise, model_kwargs, skip_timesteps, init_image,
                               dump_steps, const_noise, 0.0, step_noise, seed, draw_base, clip_denoised, clip_streams=clip_streams)
        return self._generic_loop(False, model, shape, noise, model_kwargs, skip_timesteps, init_image, dump_steps,
                                  const_noise, 0.0, device, clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                  clip_streams=clip_streams)

    PROGRESSIVE_CHUNK = 50      # steps per library call of the generator forms

    def _progressive(self, ddim, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, skip_timesteps,
                     init_image, randomize_class, cond_fn_with_grad, const_noise, eta, clip_streams=None):
        """Generator form of the loops: one {"sample": x_{t-1}} per denoising step, in loop order -- LAZY like the reference's
        (gaussian_diffusion.py:673-740): the chain runs inside the library PROGRESSIVE_CHUNK steps per call (dsg_sample_args.first_step
        / max_steps: a chain in pieces, every step of the piece dumped), so the host holds one chunk of samples at a time (round-3
        advisor: the whole chain used to be materialised, 0.4 GB at ZEGGS dims and batch 1) and a caller that abandons the generator
        stops the work.  Same samples, bit for bit, as the one-call loops: draw indices are those of the whole chain, reserved HERE,
        when the generator is created (round-4 advisor: a generator body runs at the first next(), so reserving them inside it let a
        loop started between creation and first use draw the same noise).  The seed, the stream id and `clip_streams` are captured
        with them: a `manual_seed()` between creation and the first next(), or between two chunks, does not touch a running chain."""
        hooks = self._check_unsupported(denoised_fn, cond_fn, randomize_class, cond_fn_with_grad)
        inner, guided = (None, False) if hooks else self._library_model(model, shape[0])
        n_run = self.num_timesteps - skip_timesteps
        # the generator owns these draw indices from the moment it is created -- the fused path AND (round-5 advisor) the generic path
        # (hooks / a wrapped model): noise indices are fixed here, not at the first next()
        draw0 = self._draw
        self._draw += 1 + n_run
        if clip_streams is not None:
            _clip_streams(clip_streams, int(shape[0]))      # (a wrong list fails here, not at the first next())
            clip_streams = list(clip_streams)
        owned = (self._seed & _U64, self.stream_id, clip_streams)
        return self._progressive_gen(ddim, model, inner, guided, shape, noise, clip_denoised, model_kwargs, device, skip_timesteps,
                                     init_image, const_noise, eta, n_run, draw0, denoised_fn, cond_fn, owned)

    def _progressive_gen(self, ddim, model, inner, guided, shape, noise, clip_denoised, model_kwargs, device, skip_timesteps,
                         init_image, const_noise, eta, n_run, draw0, denoised_fn=None, cond_fn=None, owned=None):
        seed, stream_id, clip_streams = owned if owned is not None else (self._seed & _U64, self.stream_id, None)
        if inner is None:
            # LAZY like the fused form: one step per next() (the whole chain used to run, and every step be cloned on the device -- 0.4 GB per
            # clip at ZEGGS dims -- before the first yield; an abandoned generator now stops the work)
            for o in self._generic_steps(ddim, model, shape, noise, model_kwargs, skip_timesteps, init_image, const_noise, eta, device,
                                         clip_denoised, denoised_fn, cond_fn, draw0, seed, stream_id, clip_streams):
                yield {"sample": o}
            return
        mode = L.MODE_DDIM if ddim else L.MODE_DDPM
        x, first = noise, 0
        while first < n_run:
            k = min(self.PROGRESSIVE_CHUNK, n_run - first)
            outs = self._fused(mode, inner, guided, shape, x, model_kwargs, skip_timesteps, init_image if first == 0 else None,
                               list(range(first, first + k)), const_noise, eta, None, seed, draw0, clip_denoised, first_step=first, max_steps=k,
                               stream_id=stream_id, clip_streams=clip_streams)
            for o in outs:
                yield {"sample": o}
            x, first = outs[-1], first + k

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                                  randomize_class=False, cond_fn_with_grad=False, const_noise=False, *, clip_streams=None):
        """`GaussianDiffusion.p_sample_loop_progressive` (gaussian_diffusion.py:673-740): yields a dict per step; key "sample"
        (the reference's "pred_xstart" is not produced: no caller on the path reads it)."""
        return self._progressive(False, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, skip_timesteps,
                                 init_image, randomize_class, cond_fn_with_grad, const_noise, 0.0, clip_streams)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, skip_timesteps=0, init_image=None,
                                     randomize_class=False, cond_fn_with_grad=False, *, clip_streams=None):
        """`GaussianDiffusion.ddim_sample_loop_progressive` (gaussian_diffusion.py:938-1003)."""
        return self._progressive(True, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, skip_timesteps,
                                 init_image, randomize_class, cond_fn_with_grad, False, eta, clip_streams)

    def p_sample_loop_multi(self, models, shape, model_kwargs_list, *, seeds=None, stream_ids=None, clip_denoised=False,
                            skip_timesteps=0, init_images=None, noises=None, ddim=False, eta=0.0, clip_streams=None):
        """`p_sample_loop` (or `ddim_sample_loop`) for SEVERAL lanes at once -- one `DSGDenoiser` per lane (a model and its
        `clone()`s: one copy of the weights), one independent sampling problem each, advanced concurrently inside the
        library (dsg_sample_multi: every lane owns an HSA queue; "one clip per stream").  Lane i draws from the Philox stream
        (seeds[i], stream_ids[i]) at this object's current draw counter, which advances once for all lanes -- so lane i
        reproduces `manual_seed(seeds[i], stream_ids[i])` + the same sequence of single-lane calls ON THE SAME LANE bit for
        bit: every lane runs the kernel set of its own handle (`DSGDenoiser.set_kernel_set`), the call itself changes nothing
        about the arithmetic.  `clip_streams`: one list per lane (B stream ids or B (seed, stream_id) pairs, as `p_sample_loop`
        takes them; an entry may be None) -- the elements of that lane draw from their own streams, `stream_ids[i]` is then unused."""
        models = list(models)
        n = len(models)
        if n == 0 or len(model_kwargs_list) != n:
            raise ValueError("one model_kwargs per lane")
        if clip_streams is not None and len(clip_streams) != n:
            raise ValueError(f"clip_streams: {len(clip_streams)} lists for {n} lanes (one list of B streams per lane)")
        seeds = [self._seed] * n if seeds is None else list(seeds)
        stream_ids = [self.stream_id + i for i in range(n)] if stream_ids is None else list(stream_ids)
        B = int(shape[0])
        args = (L.dsg_sample_args * n)()
        outs, keeps, use_torch = [], [], False
        models, guided = _inner_lanes(models, "p_sample_loop_multi", shape[0])
        for i, m in enumerate(models):
            a, keep, _, ut = self._prepare(L.MODE_DDIM if ddim else L.MODE_DDPM, m, guided[i], shape,
                                           None if noises is None else noises[i], model_kwargs_list[i], skip_timesteps,
                                           None if init_images is None else init_images[i], None, False, eta, None,
                                           seeds[i], None, clip_denoised, stream_id=stream_ids[i])
            args[i] = a
            keeps.append(keep)
            use_torch = use_torch or ut
        hs = (C.c_void_p * n)(*[m.handle for m in models])
        optrs = (C.c_void_p * n)()
        for i, m in enumerate(models):
            o, p = m._alloc_out(shape, use_torch)
            outs.append(o)
            optrs[i] = p
        lib = models[0].lib
        with _keyed(models, [None] * n if clip_streams is None else clip_streams, B):
            lib.check(lib.cdll.dsg_sample_multi(hs, n, args, optrs, B, L.current_stream_ptr() if use_torch else None))
        self._draw += 1 + (self.num_timesteps - skip_timesteps)
        self._last_model = models[0]
        return outs

    # ---- a whole clip per library call (dsg_sample_clip): the window loops of sample.py inside the library -----------------
    def sample_clip(self, model, feats, style, *, seed0=None, root_shift, keep_last_tail, ddim=False, eta=0.0, skip_timesteps=0,
                    clip_denoised=False, scale=None, seed_last=None, mask_local="ones", inpainting_mask=None, inpainted_motion=None,
                    init_motion=None, clip_streams=None):
        """All K windows of B clips in ONE library call: per-window conditioning, step loop, seed hand-off, root shift (`root_shift`,
        the ZEGGS loop's `smoothing`), one-frame blend and stitching on the device (k_window_handoff).  `feats`: the K per-window
        features exactly as y['audio'] takes them, each [B, T_a, A_src] (stacked once into [K, B, T_a, A_src]); `style` [B, style_dim_in];
        `seed0` [B, J, 1, S] = y['seed'] of window 0 (None: zeros); `scale` [B]: classifier-free guidance as y['scale'] (`model` is then
        the ClassifierFreeSampleModel, or a DSGDenoiser with room for the twins); `seed_last`: y['seed_last'] of DiffuseStyleGesture++.
        Returns the stitched clips [B, n_out, J] (numpy float32): n_out = K * stride - S (`keep_last_tail=False`, ZEGGS) or K * stride
        (`True`, DSG+: last window whole, first S frames dropped).  Bit-identical to K `p_sample_loop` / `ddim_sample_loop` calls + the
        host stitching of sample.py, and the draw counter advances as theirs does: by K * (1 + n_run).
        `inpainting_mask` / `inpainted_motion` [B, n_out, J] (numpy or torch; both or neither): motion inpainting over the whole clip, in
        the coordinates of the returned clip -- every window runs with the y['inpainting_mask'] / y['inpainted_motion'] that
        `sample.window_constraint` cuts out of them, cut on the device (`DSGDenoiser.set_clip_inpainting`; set before the call, cleared
        after it).
        `init_motion` [B, n_out, J] (numpy or torch): an existing clip to edit, in the coordinates of the returned clip -- every window
        starts from q_sample of its slice (`sample.window_init`: the `init_image` of that window's loop) instead of pure noise, noised to
        the first timestep `skip_timesteps` leaves; cut, noised and written as the sampler state by one kernel per window
        (`DSGDenoiser.set_clip_init`; set before the call, cleared after it).
        `clip_streams`: B stream ids or B (seed, stream_id) pairs, as `p_sample_loop` takes them -- clip b draws every window from its
        own Philox stream and equals the clip sampled alone (`DSGDenoiser.set_noise_streams`; set before the call, cleared after it)."""
        if (inpainting_mask is None) != (inpainted_motion is None):
            raise ValueError("sample_clip: inpainting_mask and inpainted_motion go together")
        return self.sample_clip_multi([model], [feats], [style], seed0s=None if seed0 is None else [seed0], root_shift=root_shift,
                                      keep_last_tail=keep_last_tail, ddim=ddim, eta=eta, skip_timesteps=skip_timesteps,
                                      clip_denoised=clip_denoised, scales=None if scale is None else [scale],
                                      seed_lasts=None if seed_last is None else [seed_last], mask_local=mask_local,
                                      stream_ids=[self.stream_id], inpainting_masks=None if inpainting_mask is None else [inpainting_mask],
                                      inpainted_motions=None if inpainted_motion is None else [inpainted_motion],
                                      init_motions=None if init_motion is None else [init_motion],
                                      clip_streams=None if clip_streams is None else [clip_streams])[0]

    def sample_clip_multi(self, models, feats_per_lane, styles, *, seed0s=None, root_shift, keep_last_tail, ddim=False, eta=0.0,
                          skip_timesteps=0, clip_denoised=False, scales=None, seed_lasts=None, mask_local="ones", seeds=None,
                          stream_ids=None, inpainting_masks=None, inpainted_motions=None, init_motions=None, clip_streams=None):
        """`sample_clip` for several lanes at once (dsg_sample_clip_multi; lanes as in `p_sample_loop_multi`): lane i samples the B
        clips of feats_per_lane[i] from the Philox stream (seeds[i], stream_ids[i]); the windows advance in lock step over the lanes.
        `inpainting_masks` / `inpainted_motions`: one [B, n_out, J] pair per lane, entries may be None (that lane runs unconstrained).
        `init_motions`: one [B, n_out, J] clip per lane to start from, entries may be None (that lane starts from noise).
        `clip_streams`: one list of B streams per lane as in `p_sample_loop_multi`, entries may be None.
        Returns one [B, n_out, J] array per lane."""
        models = list(models)
        n = len(models)
        if n == 0 or len(feats_per_lane) != n or len(styles) != n:
            raise ValueError("one feature list and one style batch per lane")
        if (inpainting_masks is None) != (inpainted_motions is None):
            raise ValueError("sample_clip: inpainting_masks and inpainted_motions go together")
        inp = [(None, None)] * n if inpainting_masks is None else list(zip(inpainting_masks, inpainted_motions))
        if len(inp) != n or any((mk is None) != (mo is None) for mk, mo in inp):
            raise ValueError("sample_clip: one inpainting mask and one motion per lane (or None for both)")
        inits = [None] * n if init_motions is None else list(init_motions)
        if len(inits) != n:
            raise ValueError("sample_clip: one init motion per lane (or None)")
        if clip_streams is not None and len(clip_streams) != n:
            raise ValueError(f"clip_streams: {len(clip_streams)} lists for {n} lanes (one list of B streams per lane)")
        K = len(feats_per_lane[0])
        if K < 1 or any(len(f) != K for f in feats_per_lane):
            raise ValueError("the same number of windows (>= 1) for every lane")
        seeds = [self._seed] * n if seeds is None else list(seeds)
        stream_ids = [self.stream_id + i for i in range(n)] if stream_ids is None else list(stream_ids)
        use_torch = L.is_torch(feats_per_lane[0][0])
        B = int(feats_per_lane[0][0].shape[0])
        inners, guided = _inner_lanes(models, "sample_clip", B)
        if any(guided) and scales is None:
            raise KeyError("scale")
        cfg = inners[0].cfg
        S, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
        n_run = self.num_timesteps - skip_timesteps
        n_out = K * (T - S) - (0 if keep_last_tail else S)
        if isinstance(mask_local, str):
            if use_torch:
                import torch
                mask_local = torch.ones(1, T, dtype=torch.uint8, device=feats_per_lane[0][0].device)
            else:
                mask_local = np.ones((1, T), np.uint8)
        mbuf = L.Buf(mask_local, "uint8") if mask_local is not None else L.Buf(None)
        mb = 0 if mask_local is None else (int(mbuf.obj.shape[0]) if mbuf.obj.ndim == 2 else 1)
        stream = L.current_stream_ptr() if use_torch else None
        args = (L.dsg_sample_args * n)()
        keep, outs = [mbuf], []
        ptrs = {k: (C.c_void_p * n)() for k in ("h", "style", "seed0", "audio", "scale", "out")}
        for i, m in enumerate(inners):
            if m.inpainting:
                raise ValueError("sample_clip: an inpainting constraint is per window (the host window loop takes it)")
            m.set_schedule(self)
            if use_torch:
                import torch
                audio = L.Buf(torch.stack([f.float() for f in feats_per_lane[i]]))
            else:
                audio = L.Buf(np.stack([np.asarray(f, np.float32) for f in feats_per_lane[i]]))
            if tuple(audio.obj.shape) != (K, B, cfg.audio_frames, cfg.audio_src_dim):
                raise ValueError(f"feats shape {tuple(audio.obj.shape)} != {(K, B, cfg.audio_frames, cfg.audio_src_dim)}")
            style = L.Buf(styles[i])
            if tuple(style.obj.shape) != (B, cfg.style_dim_in):
                raise ValueError(f"style shape {tuple(style.obj.shape)}")
            seed0 = L.Buf(None if seed0s is None else seed0s[i])
            if seed0.obj is not None and tuple(seed0.obj.shape) != (B, J, 1, S):
                raise ValueError(f"seed0 shape {tuple(seed0.obj.shape)}")
            sc = L.Buf(None if scales is None else scales[i])
            if sc.obj is not None:
                if int(np.prod(sc.obj.shape)) != B:
                    raise ValueError(f"scale must have {B} entries")
                if m.max_batch < 2 * B:
                    raise ValueError(f"classifier-free guidance runs the unconditional twins in the same batch: max_batch >= {2 * B}")
            if cfg.variant == 5:
                if seed_lasts is None or seed_lasts[i] is None:
                    raise KeyError("seed_last")
                last = L.Buf(seed_lasts[i])
                if tuple(last.obj.shape) != (B, J, 1, S):
                    raise ValueError(f"seed_last shape {tuple(last.obj.shape)}")
                m.lib.check(m.lib.cdll.dsg_set_seed_last(m.handle, last.p, B, stream))
                keep.append(last)
            args[i] = self._clip_args(ddim, eta, skip_timesteps, clip_denoised, seeds[i], stream_ids[i])
            if use_torch and audio.obj.is_cuda:      # device -> PINNED host memory, as sample.py's _zeggs_finish
                import torch
                out = torch.empty((B, n_out, J), dtype=torch.float32, pin_memory=True)
                optr = out.data_ptr()
                out = out.numpy()
            else:
                out = np.empty((B, n_out, J), np.float32)
                optr = out.ctypes.data
            outs.append(out)
            keep += [audio, style, seed0, sc]
            for k, v in (("h", m.handle), ("style", style.ptr), ("seed0", seed0.ptr), ("audio", audio.ptr), ("scale", sc.ptr), ("out", optr)):
                ptrs[k][i] = v
        lib = inners[0].lib
        keyed = _keyed(inners, [None] * n if clip_streams is None else clip_streams, B)
        try:
            with keyed:
                for m, (mk, mo) in zip(inners, inp):
                    if mk is not None:
                        if tuple(mo.shape) != (B, n_out, J):
                            raise ValueError(f"clip inpainted_motion shape {tuple(mo.shape)} != {(B, n_out, J)}")
                        m.set_clip_inpainting(mk, mo, B)
                    elif m.clip_inpainting:
                        m.set_clip_inpainting(None, None, 0)
                for m, init in zip(inners, inits):
                    if init is not None:
                        if tuple(init.shape) != (B, n_out, J):
                            raise ValueError(f"clip init_motion shape {tuple(init.shape)} != {(B, n_out, J)}")
                        m.set_clip_init(init, B)
                    elif m.clip_init:
                        m.set_clip_init(None, 0)
                if n == 1:
                    lib.check(lib.cdll.dsg_sample_clip(ptrs["h"][0], ptrs["style"][0], ptrs["seed0"][0], ptrs["audio"][0], mbuf.p, mb,
                                                       ptrs["scale"][0], C.byref(args[0]), K, int(bool(root_shift)), int(bool(keep_last_tail)),
                                                       ptrs["out"][0], B, stream))
                else:
                    lib.check(lib.cdll.dsg_sample_clip_multi(ptrs["h"], n, ptrs["style"], ptrs["seed0"], ptrs["audio"], mbuf.p, mb, ptrs["scale"],
                                                             args, K, int(bool(root_shift)), int(bool(keep_last_tail)), ptrs["out"], B, stream))
        finally:
            for m in inners:
                if m.clip_inpainting:
                    m.set_clip_inpainting(None, None, 0)
                if m.clip_init:
                    m.set_clip_init(None, 0)
        self._draw += K * (1 + n_run)
        self._last_model = inners[0]
        return outs

    # ---- clips of different lengths over one batch of slots (dsg_sample_clip_queue) ------------------------------------------
    @staticmethod
    def _clip_queue_job(cfg, clip, i, job, edit, use_torch, keep_last_tail, seed, who="sample_clip_queue", capacity=None):
        """One clip dict of `sample_clip_queue` / `ClipQueue.submit` as the library's dsg_clip_job + dsg_clip_edit (filled in place).  Returns
        (the host `out` [n_out, J], the buffers that must outlive the call, whether the clip has an edit).  `seed`: the seed of a clip whose
        "stream" is a bare id.  `capacity` (`submit_live`): the job's K and the size of `out`; "feats" are the windows given so far and may
        be empty."""
        from .model import _mask_bytes
        S, T, J = cfg.n_seed, cfg.n_poses, cfg.njoints
        edit_keys = ("inpainting_mask", "inpainted_motion", "init_motion")
        feats = list(clip.get("feats") or []) if capacity is not None else list(clip["feats"])
        if not feats and capacity is None:
            raise ValueError(f"{who}: a clip without windows")
        if not feats:
            audio = L.Buf(None)
        elif use_torch:
            import torch
            audio = L.Buf(torch.stack([f.float().reshape(cfg.audio_frames, cfg.audio_src_dim) for f in feats]))
        else:
            audio = L.Buf(np.stack([np.asarray(f, np.float32).reshape(cfg.audio_frames, cfg.audio_src_dim) for f in feats]))
        style = L.Buf(clip["style"])
        if int(np.prod(style.obj.shape)) != cfg.style_dim_in:
            raise ValueError(f"style shape {tuple(style.obj.shape)}")
        seed0, last = L.Buf(clip.get("seed0")), L.Buf(clip.get("seed_last"))
        for name, b in (("seed0", seed0), ("seed_last", last)):
            if b.obj is not None and int(np.prod(b.obj.shape)) != J * S:
                raise ValueError(f"{name} shape {tuple(b.obj.shape)}")
        st = clip.get("stream", 0)
        sd, sid = (st if isinstance(st, (tuple, list)) else (seed, st))
        K = len(feats) if capacity is None else int(capacity)
        out = np.empty((max(K * (T - S) - (0 if keep_last_tail else S), 0), J), np.float32)
        job.style, job.seed0, job.seed_last, job.audio, job.out = style.ptr, seed0.ptr, last.ptr, audio.ptr, out.ctypes.data
        job.K, job.scale = K, float(1.0 if clip.get("scale") is None else clip["scale"])
        job.seed, job.stream_id = int(sd) & _U64, int(sid) & _U64
        mk, mo, init = (clip.get(k) for k in edit_keys)
        if (mk is None) != (mo is None):
            raise ValueError(f"{who}: clip {i}: inpainting_mask and inpainted_motion go together")
        bufs = [L.Buf(None if mk is None else _mask_bytes(mk), "uint8"), L.Buf(mo), L.Buf(init)]
        for name, b in zip(edit_keys, bufs):
            if b.obj is not None and tuple(b.obj.shape) not in (out.shape, (1,) + out.shape):
                raise ValueError(f"{who}: clip {i}: {name} shape {tuple(b.obj.shape)} != {out.shape}")
        edit.inp_mask, edit.inp_motion, edit.init_motion = (b.ptr for b in bufs)
        return out, [audio, style, seed0, last] + bufs, any(b.obj is not None for b in bufs)

    def sample_clip_queue(self, lanes, clips, B, *, root_shift, keep_last_tail, ddim=False, eta=0.0, skip_timesteps=0, clip_denoised=False,
                          guided=False, mask_local="ones"):
        """N clips of their own lengths over `lanes` x `B` slots in ONE library call: a slot is refilled when its clip ends
        (`lib.clip_queue_plan` is the schedule).  `lanes`: a DSGDenoiser (or the ClassifierFreeSampleModel around one) or a list of them.
        `clips`: one dict per clip -- "feats": its K_i per-window features exactly as y['audio'] takes them, each [T_a, A_src] (or
        [1, T_a, A_src]); "style" [style_dim_in]; "stream": its stream id, or a (seed, stream_id) pair (a bare id keeps the seed of
        `manual_seed`); optional "seed0" [J, 1, S] = y['seed'] of window 0 (None: zeros), "seed_last" (DiffuseStyleGesture++), "scale"
        (`guided=True`: y['scale'] of the clip, default 1).  Returns one [n_out_i, J] numpy array per clip, in the order given; clip i is bit
        for bit `sample_clip` of that clip alone (batch 1) after `manual_seed(seed_i, stream_i)` under the same kernel set.  The draw counter
        advances by max(K_i) * (1 + n_run), as the longest clip alone would advance it.
        Per-clip edits, three more optional keys (numpy or torch, host or device): "inpainting_mask" / "inpainted_motion" (both or
        neither) and "init_motion", each [n_out_i, J] or [1, n_out_i, J] in the coordinates of the clip returned -- what `sample_clip`
        takes as `inpainting_mask` / `inpainted_motion` / `init_motion` for that clip alone, and clip i is bit for bit that call.  They
        travel with the clip (dsg_sample_clip_queue_edit, called only when some clip has one); a clip without them beside clips with
        some comes out as it does without.
        Per-clip strength: a clip may carry "skip_timesteps" (0 .. num_timesteps - 1); the keyword is the default for clips without one.
        Clip i is then bit for bit `sample_clip` of that clip alone with ITS skip_timesteps, so fresh generations (0) and edits of any
        depth share the slots of one call (dsg_sample_clip_queue_steps, called only when some clip has the key; `lib.clip_queue_plan`
        with `n_run` is the schedule).  The draw counter advances by max(K_i * (1 + n_run_i))."""
        inners, _ = _inner_lanes(lanes, "sample_clip_queue")
        clips = list(clips)
        if not inners or not clips:
            raise ValueError("sample_clip_queue: at least one lane and one clip")
        cfg = inners[0].cfg
        skips, own_skips = [], False
        for i, clip in enumerate(clips):
            sk = clip.get("skip_timesteps")
            if sk is None:      # (the keyword: checked by the library, as in a call without the key)
                skips.append(int(skip_timesteps))
                continue
            own_skips = True
            if not 0 <= int(sk) < self.num_timesteps:
                raise ValueError(f"sample_clip_queue: clip {i}: skip_timesteps {int(sk)} outside [0, {self.num_timesteps - 1}]")
            skips.append(int(sk))
        use_torch = L.is_torch(clips[0]["feats"][0])
        edit_keys = ("inpainting_mask", "inpainted_motion", "init_motion")
        stream = L.current_stream_ptr() if use_torch or any(L.is_torch(c.get(k)) for c in clips for k in edit_keys) else None
        mbuf = _queue_mask(mask_local, cfg.n_poses, "sample_clip_queue")
        jobs = (L.dsg_clip_job * len(clips))()
        edits, edited = (L.dsg_clip_edit * len(clips))(), False
        keep, outs = [mbuf], []
        for i, (job, edit, clip) in enumerate(zip(jobs, edits, clips)):
            out, bufs, has_edit = self._clip_queue_job(cfg, clip, i, job, edit, use_torch, keep_last_tail, self._seed)
            edited = edited or has_edit
            keep += bufs
            outs.append(out)
        for m in inners:
            m.set_schedule(self)
        a = self._clip_args(ddim, eta, skip_timesteps, clip_denoised)
        hs = (C.c_void_p * len(inners))(*[m.handle for m in inners])
        lib = inners[0].lib
        tail = (int(B), mbuf.p, int(bool(guided)), C.byref(a), int(bool(root_shift)), int(bool(keep_last_tail)), stream)
        if own_skips:
            sk = np.asarray(skips, np.int32)
            lib.check(lib.cdll.dsg_sample_clip_queue_steps(hs, len(inners), jobs, edits if edited else None, sk.ctypes.data, len(clips), *tail))
        elif edited:
            lib.check(lib.cdll.dsg_sample_clip_queue_edit(hs, len(inners), jobs, edits, len(clips), *tail))
        else:
            lib.check(lib.cdll.dsg_sample_clip_queue(hs, len(inners), jobs, len(clips), *tail))
        self._draw += max(int(j.K) * (1 + self.num_timesteps - sk) for j, sk in zip(jobs, skips))
        self._last_model = inners[0]
        return outs

    def open_clip_queue(self, lanes, B, *, root_shift, keep_last_tail, ddim=False, eta=0.0, skip_timesteps=0, clip_denoised=False, guided=False,
                        mask_local="ones"):
        """The clip queue as a session (dsg_queue_*): a `ClipQueue` over `lanes` x `B` slots that takes clips while it runs and hands their
        rows back window by window.  The arguments are those of `sample_clip_queue` without the clips; `guided` is fixed for the session,
        every clip runs at its own "scale".  Use it as a context manager: the lanes belong to the session until it is closed.  Every clip
        is bit for bit `sample_clip` of that clip alone, whenever it was submitted.  `draw_base` is this diffusion's counter at open; at
        close the counter advances by the largest K * (1 + n_run) submitted, as the longest clip alone would advance it."""
        return ClipQueue(self, lanes, B, root_shift=root_shift, keep_last_tail=keep_last_tail, ddim=ddim, eta=eta, skip_timesteps=skip_timesteps,
                         clip_denoised=clip_denoised, guided=guided, mask_local=mask_local)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, skip_timesteps=0, init_image=None,
                         randomize_class=False, cond_fn_with_grad=False, dump_steps=None, const_noise=False,
                         *, step_noise=None, seed=None, draw_base=None, clip_streams=None):
        if dump_steps is not None:
            raise NotImplementedError()
        if const_noise:
            raise NotImplementedError()
        hooks = self._check_unsupported(denoised_fn, cond_fn, randomize_class, cond_fn_with_grad)
        inner, guided = (None, False) if hooks else self._library_model(model, shape[0])
        if inner is not None:
            return self._fused(L.MODE_DDIM, inner, guided, shape, noise, model_kwargs, skip_timesteps, init_image, None,
                               False, eta, step_noise, seed, draw_base, clip_denoised, clip_streams=clip_streams)
        return self._generic_loop(True, model, shape, noise, model_kwargs, skip_timesteps, init_image, None, False,
                                  eta, device, clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn, clip_streams=clip_streams)

    def last_step_time_us(self):
        """GPU time per denoising step of the last fused call (HIP events inside the library)."""
        m = getattr(self, "_last_model", None)
        if m is None:
            return None
        ms, n = C.c_float(), C.c_int()
        m.lib.check(m.lib.cdll.dsg_last_sample_ms(m.handle, C.byref(ms), C.byref(n)))
        return 1000.0 * ms.value / max(n.value, 1)

    def last_sample_path(self):
        """"hip" / "aql" / "graph": how the library submitted the step loop of the last fused call."""
        m = getattr(self, "_last_model", None)
        return None if m is None else m.last_sample_path()

    # ---- generic loop: any callable model, fused HIP elementwise kernels for the sampler arithmetic --------------
    def _f32(self, name, idx, B):
        return np.full((B,), np.float32(getattr(self, name)[idx]), dtype=np.float32)

    def _generic_loop(self, ddim, model, shape, noise, model_kwargs, skip_timesteps, init_image, dump_steps,
                      const_noise, eta, device, clip_denoised=False, denoised_fn=None, cond_fn=None, clip_streams=None):
        """The generic loop run to its end: the last sample, or clones of the samples after the steps listed in `dump_steps`."""
        n_run = self.num_timesteps - skip_timesteps
        draw0 = self._draw
        self._draw += 1 + n_run
        img, dump = None, []
        for n, img in enumerate(self._generic_steps(ddim, model, shape, noise, model_kwargs, skip_timesteps, init_image, const_noise, eta,
                                                    device, clip_denoised, denoised_fn, cond_fn, draw0, self._seed & _U64, self.stream_id,
                                                    clip_streams)):
            if dump_steps is not None and n in dump_steps:
                dump.append(img.clone())
        return dump if dump_steps is not None else img

    def _generic_steps(self, ddim, model, shape, noise, model_kwargs, skip_timesteps, init_image, const_noise, eta, device,
                       clip_denoised, denoised_fn, cond_fn, draw0, seed, stream_id, clip_streams=None):
        """Generator: x_{t-1} after every step of the loop, any callable as the denoiser; draw indices draw0 (x_T), draw0 + 1 + n (step n) --
        reserved by the caller, like `seed` / `stream_id` / `clip_streams`: a generator body runs at the first next(), and the chain draws
        from the streams the object had when the loop was created.  The noise is the framework's Philox stream (dsg_noise; with
        `clip_streams` dsg_noise_streams: every element its own stream, with `const_noise` element 0's for everyone), draw for draw the one the
        fused loop consumes -- a wrapped model keeps seed parity with the fused path and the oracle.  `denoised_fn(x0)` is applied to the
        prediction before the clamp (gaussian_diffusion.py:364-370); `cond_fn(x_t, t, **model_kwargs)` -- t the MODEL timesteps, as the wrapped
        cond_fn of SpacedDiffusion sees them (respace.py:117-129) -- shifts the DDPM mean by posterior_variance * grad (condition_mean, :428-441)
        and the DDIM eps by -sqrt(1 - alpha_bar) * grad (condition_score, :458-480)."""
        import torch
        lib = self._lib or L.default_library()
        if device is None:
            device = next(model.parameters()).device
        # gaussian_diffusion.py:317-321 (both keys, as in `_prepare`); the shapes are checked before any work is done
        inp_mask = inp_motion = None
        y = (model_kwargs or {}).get("y") or {}
        if _INPAINT_KEYS[0] in y and _INPAINT_KEYS[1] in y:
            inp_mask = torch.as_tensor(_inpaint_mask(y[_INPAINT_KEYS[0]]))
            inp_motion = torch.as_tensor(y[_INPAINT_KEYS[1]])
            for key, v in zip(_INPAINT_KEYS, (inp_mask, inp_motion)):
                if tuple(v.shape) != tuple(shape):
                    raise ValueError(f"y['{key}'] shape {tuple(v.shape)} != {tuple(shape)}")
            inp_mask, inp_motion = inp_mask.to(device), inp_motion.to(device=device, dtype=torch.float32)
        B = int(shape[0])
        per = int(np.prod(shape[1:]))
        stream = L.current_stream_ptr()
        keys = None
        if clip_streams is not None:
            seeds, ids = _clip_streams(clip_streams, B)
            seeds = [seed] * B if seeds is None else seeds
            if const_noise:
                seeds, ids = [seeds[0]] * B, [ids[0]] * B
            keys = (np.array(seeds, dtype=np.uint64), np.array(ids, dtype=np.uint64))

        def z(draw):
            t = torch.empty(*shape, device=device, dtype=torch.float32)
            if keys is not None:
                lib.check(lib.cdll.dsg_noise_streams(t.data_ptr(), B, int(shape[1]) * int(shape[2]), int(shape[3]), keys[0].ctypes.data,
                                                     keys[1].ctypes.data, draw, stream))
            else:
                lib.check(lib.cdll.dsg_noise(t.data_ptr(), B, int(shape[1]) * int(shape[2]), int(shape[3]), seed, stream_id, draw, stream))
            return t
        img = noise if noise is not None else z(draw0)      # (the x_T draw index is reserved either way, as in the fused loop)
        if skip_timesteps and init_image is None:
            init_image = torch.zeros_like(img)
        indices = list(range(self.num_timesteps - skip_timesteps))[::-1]
        if init_image is not None:
            out = torch.empty_like(img)
            init_c, img_c = init_image.contiguous(), img.contiguous()
            # (host coefficient arrays are bound to names: a temporary's `.ctypes.data` dangles once the expression is done)
            qa, qb = self._f32("sqrt_alphas_cumprod", indices[0], B), self._f32("sqrt_one_minus_alphas_cumprod", indices[0], B)
            lib.check(lib.cdll.dsg_q_sample(out.data_ptr(), init_c.data_ptr(), img_c.data_ptr(), qa.ctypes.data, qb.ctypes.data,
                                            B, per, stream))
            img = out
        tmap = torch.tensor(self.timestep_map, device=device, dtype=torch.long)
        for n, i in enumerate(indices):
            t = torch.full((B,), i, device=device, dtype=torch.long)
            with torch.no_grad():
                x0 = model(img, tmap[t], **(model_kwargs or {})).contiguous().float()
                if inp_mask is not None:      # gaussian_diffusion.py:317-321: before denoised_fn and the clamp
                    x0 = torch.where(inp_mask, inp_motion, x0)
                if denoised_fn is not None:
                    x0 = denoised_fn(x0).contiguous().float()
                if clip_denoised:
                    x0 = x0.clamp(-1, 1)
                grad = None if cond_fn is None else cond_fn(img, tmap[t], **(model_kwargs or {})).float()
            eps = z(draw0 + 1 + n)
            if const_noise:
                eps = eps[[0]].repeat(B, 1, 1, 1)
            nz = np.float32(0.0 if i == 0 else 1.0)
            out = torch.empty_like(img)
            img = img.contiguous()
            if not ddim:
                sig = nz * np.exp(np.float32(0.5) * np.float32(self.posterior_log_variance_clipped[i]))
                c1, c2 = self._f32("posterior_mean_coef1", i, B), self._f32("posterior_mean_coef2", i, B)
                c3 = np.full((B,), sig, np.float32)
                lib.check(lib.cdll.dsg_posterior_step(out.data_ptr(), x0.data_ptr(), img.data_ptr(), eps.data_ptr(),
                                                      c1.ctypes.data, c2.ctypes.data, c3.ctypes.data, B, per, stream))
                if grad is not None:
                    out = out + float(np.float32(self.posterior_variance[i])) * grad
            else:
                ab, abp = np.float32(self.alphas_cumprod[i]), np.float32(self.alphas_cumprod_prev[i])
                one = np.float32(1)
                if grad is not None:
                    rc, rm = float(np.float32(self.sqrt_recip_alphas_cumprod[i])), float(np.float32(self.sqrt_recipm1_alphas_cumprod[i]))
                    e = (rc * img - x0) / rm - float(np.sqrt(one - ab)) * grad
                    x0 = (rc * img - rm * e).contiguous()
                sigma = np.float32(eta) * np.sqrt((one - abp) / (one - ab)) * np.sqrt(one - ab / abp)
                coef = np.tile(np.array([np.float32(self.sqrt_recip_alphas_cumprod[i]),
                                         np.float32(self.sqrt_recipm1_alphas_cumprod[i]), np.sqrt(abp),
                                         np.sqrt(one - abp - sigma * sigma), nz * sigma], np.float32), (B, 1))
                coef = np.ascontiguousarray(coef)
                lib.check(lib.cdll.dsg_ddim_step(out.data_ptr(), x0.data_ptr(), img.data_ptr(), eps.data_ptr(),
                                                 coef.ctypes.data, B, per, stream))
            img = out
            yield img


_INPAINT_KEYS = ("inpainting_mask", "inpainted_motion")


class _JobInfo(dict):
    """what `ClipQueue.job` returns: a dict in which the words of parking read as their defaults while they are not stored"""
    DEFAULTS = {"parks": 0, "held": False, "priority": 0}

    def __missing__(self, key):
        return self.DEFAULTS[key]


class ClipQueue:
    """A queue session (`DSGDiffusion.open_clip_queue`; dsg_queue_* of include/dsg.h).  `submit` a clip dict at any time, `run` rounds,
    read `rows(ticket)` as windows finish, `result(ticket)` when the clip is done.  Host tensors of a clip are copied by `submit`; device
    tensors must stay valid until the clip is done or cancelled (the session keeps a reference).  Not thread safe: submit and run from
    one thread.  Placement is by priority, then first come, first served: every round the waiting clips -- pending or parked, not held --
    take the free slots, highest `priority` first, oldest ticket first, and then the slots of running clips of a strictly lower priority,
    which are parked at that window boundary and continue later in any slot (`lib.queue_place_prio`; with equal priorities
    `lib.queue_place`).  `park` / `resume` pause a clip and let it go on; a clip comes out bit for bit the same however often it was parked."""

    def __init__(self, diffusion, lanes, B, *, root_shift, keep_last_tail, ddim, eta, skip_timesteps, clip_denoised, guided, mask_local):
        self._handle = None
        self.lanes, _ = _inner_lanes(lanes, "open_clip_queue")
        if not self.lanes:
            raise ValueError("open_clip_queue: at least one lane")
        self.diffusion, self.cfg, self.B, self.keep_last_tail = diffusion, self.lanes[0].cfg, int(B), bool(keep_last_tail)
        self.lib = self.lanes[0].lib
        mbuf = _queue_mask(mask_local, self.cfg.n_poses, "open_clip_queue")
        for m in self.lanes:
            m.set_schedule(diffusion)
        a = diffusion._clip_args(ddim, eta, skip_timesteps, clip_denoised)
        self.skip_timesteps = int(skip_timesteps)
        self._seed = diffusion._seed
        self._advance = 0
        self._outs, self._keep = [], {}
        self._live = {}                                  # ticket -> [windows given, steps per window] of a live job
        self._prio = []                                  # per ticket: its priority (the library reports every other word of a job)
        hs = (C.c_void_p * len(self.lanes))(*[m.handle for m in self.lanes])
        q = C.c_void_p()
        self.lib.check(self.lib.cdll.dsg_queue_open(hs, len(self.lanes), self.B, mbuf.p, int(bool(guided)), C.byref(a), int(bool(root_shift)),
                                                    int(self.keep_last_tail), C.byref(q)))
        self._handle = q

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _q(self):
        if self._handle is None:
            raise L.DSGError("the clip queue is closed")
        return self._handle

    def submit(self, clip, out=None, priority=0) -> int:
        """One clip dict as `sample_clip_queue` takes it, "skip_timesteps" and the edit keys included.  Returns its ticket (0, 1, ...).
        `out`: the caller's own C-contiguous float32 numpy array [n_out, J] to receive the clip (a playback buffer); rows past
        `rows_ready` are never touched.  Default: an array of the session's.  `priority` (or a "priority" key of the dict): higher runs
        first and takes the slot of a running clip of a lower one; default 0."""
        return self._submit(clip, out, None, priority)

    def submit_live(self, clip, capacity, out=None, priority=0) -> int:
        """A live clip (dsg_queue_submit_live): its windows arrive while it runs.  `clip` as for `submit`, without edits; "feats" are the
        windows known now and may be empty.  `capacity`: the most windows it may ever get -- `out` (the caller's, or the session's) is
        [n_out(capacity), J].  Feed it with `append`, end it with `finish` (or `append(..., last=True)`); `rows` / `result` as for every
        clip.  With K windows given it is bit for bit `sample_clip` of those K windows alone, whenever they arrived."""
        self._q()
        if any(clip.get(k) is not None for k in ("inpainting_mask", "inpainted_motion", "init_motion")):
            raise ValueError(f"ClipQueue.submit_live: clip {len(self._outs)}: a live clip takes no edits (their coordinates depend on the final length)")
        return self._submit(clip, out, capacity, priority)

    def _submit(self, clip, out, capacity, priority=0):
        """`submit` (`capacity` None: dsg_queue_submit) and `submit_live` (dsg_queue_submit_live)"""
        live = capacity is not None
        who = "ClipQueue.submit_live" if live else "ClipQueue.submit"
        q, d = self._q(), self.diffusion
        i = len(self._outs)
        sk = clip.get("skip_timesteps")
        if sk is not None and not 0 <= int(sk) < d.num_timesteps:
            raise ValueError(f"{who}: clip {i}: skip_timesteps {int(sk)} outside [0, {d.num_timesteps - 1}]")
        feats = (clip.get("feats") or []) if live else clip["feats"]
        first = feats[0] if len(feats) else None
        # (the current torch stream goes with the job as soon as ANY of its tensors is a torch tensor: the library orders its reads behind it)
        tensors = [first] + [clip.get(k) for k in ("style", "seed0", "seed_last", "inpainting_mask", "inpainted_motion", "init_motion")]
        stream = L.current_stream_ptr() if any(L.is_torch(t) for t in tensors) else None
        job, edit = L.dsg_clip_job(), L.dsg_clip_edit()
        # (a bare stream id keeps the seed the session was opened under)
        own, bufs, has_edit = d._clip_queue_job(self.cfg, clip, i, job, edit, L.is_torch(first), self.keep_last_tail, self._seed, who=who, capacity=capacity)
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == own.shape):
                raise ValueError(f"{who}: clip {i}: out must be a C-contiguous float32 array of shape {own.shape}")
            job.out = out.ctypes.data
        else:
            out = own
        ticket, skip = C.c_int64(-1), -1 if sk is None else int(sk)
        if live:
            self.lib.check(self.lib.cdll.dsg_queue_submit_live(q, C.byref(job), len(feats), skip, C.byref(ticket), stream))
        else:
            self.lib.check(self.lib.cdll.dsg_queue_submit(q, C.byref(job), C.byref(edit) if has_edit else None, skip, C.byref(ticket), stream))
        assert ticket.value == i
        self._outs.append(out)
        self._prio.append(0)
        prio = clip.get("priority")
        prio = int(priority) if prio is None else int(prio)
        if prio:
            self.set_priority(i, prio)
        dev = [b for b in bufs if b.obj is not None and L.is_torch(b.obj) and b.obj.is_cuda]
        if dev:
            self._keep[i] = dev                          # device tensors are read where they are, until the clip is done or cancelled
        steps = 1 + d.num_timesteps - (self.skip_timesteps if sk is None else int(sk))
        if live:
            self._live[i] = [0, steps]
            self._given(i, len(feats))
        else:
            self._advance = max(self._advance, int(job.K) * steps)
        return i

    def _given(self, ticket, n):
        g = self._live[ticket]
        g[0] += n
        self._advance = max(self._advance, g[0] * g[1])

    def append(self, ticket, feats, style=None, scale=None, last=False):
        """Further windows for a live clip (dsg_queue_append).  `feats`: one window [T_a, A_src] (or [1, T_a, A_src]), or a list of them.
        `style` / `scale`: from the first of these windows on (None: as before; `scale` is read by a guided session only).  `last=True`:
        `finish` in the same call.  Host arrays are copied by the call; device tensors must stay valid until their window has run."""
        q, cfg, t = self._q(), self.cfg, int(ticket)
        wins = list(feats) if isinstance(feats, (list, tuple)) else [feats]
        arr = (L.dsg_queue_window * max(len(wins), 1))()
        bufs = []
        for k, f in enumerate(wins):
            a = L.Buf(f.float().reshape(cfg.audio_frames, cfg.audio_src_dim) if L.is_torch(f)
                      else np.asarray(f, np.float32).reshape(cfg.audio_frames, cfg.audio_src_dim))
            bufs.append(a)
            arr[k].audio = a.ptr
            if k == 0 and style is not None:
                st = L.Buf(style)
                if int(np.prod(st.obj.shape)) != cfg.style_dim_in:
                    raise ValueError(f"style shape {tuple(st.obj.shape)}")
                bufs.append(st)
                arr[k].style = st.ptr
            if k == 0 and scale is not None:
                arr[k].scale, arr[k].flags = float(scale), L.WIN_SCALE
        if last and wins:
            arr[len(wins) - 1].flags |= L.WIN_LAST
        dev = [b for b in bufs if L.is_torch(b.obj) and b.obj.is_cuda]
        self.lib.check(self.lib.cdll.dsg_queue_append(q, t, arr, len(wins), L.current_stream_ptr() if dev else None))
        if dev:
            self._keep.setdefault(t, []).extend(dev)
        if t in self._live:
            self._given(t, len(wins))

    def finish(self, ticket):
        """No more windows for a live clip (dsg_queue_finish): its length is the windows given.  It is done after the round of its last
        window -- at once when that has run already."""
        self.lib.check(self.lib.cdll.dsg_queue_finish(self._q(), int(ticket)))

    def set_priority(self, ticket, priority):
        """dsg_queue_set_priority: read at the next placement; a clip that is done or cancelled keeps what it had."""
        self.lib.check(self.lib.cdll.dsg_queue_set_priority(self._q(), int(ticket), int(priority)))
        if self.job(ticket)["state"] not in (L.JOB_DONE, L.JOB_CANCELLED):
            self._prio[int(ticket)] = int(priority)

    def park(self, ticket):
        """dsg_queue_park: the clip waits -- a pending one is not placed, a running one leaves its slot at the start of the next round --
        until `resume`.  Its rows so far stay; it continues bit for bit where it stopped."""
        self.lib.check(self.lib.cdll.dsg_queue_park(self._q(), int(ticket)))

    def resume(self, ticket):
        """dsg_queue_resume: the clip competes for a slot again, like any waiting clip."""
        self.lib.check(self.lib.cdll.dsg_queue_resume(self._q(), int(ticket)))

    def run(self, max_rounds=1) -> int:
        """Up to `max_rounds` rounds (0: until nothing has a window to run and nothing pending can be placed); returns the rounds run."""
        n = C.c_int(0)
        stream = L.current_stream_ptr() if self._keep else None
        self.lib.check(self.lib.cdll.dsg_queue_run(self._q(), int(max_rounds), C.byref(n), stream))
        self.diffusion._last_model = self.lanes[0]
        for t in [t for t in self._keep if self.job(t)["state"] in (L.JOB_DONE, L.JOB_CANCELLED)]:
            del self._keep[t]
        return int(n.value)

    def job(self, ticket) -> dict:
        """{"state", "windows_done", "rows_ready", "slot", "first_round"} of a ticket (state: lib.JOB_*); a live clip adds "windows_given",
        "live" (True) and "finished".  j["parks"] (how often the clip left a slot before its end), j["held"] and j["priority"] read 0 /
        False / 0 for a clip that was never parked, held or given a priority, and are stored in the dict only once they differ: the dict
        of such a clip compares equal to what it always was."""
        info = L.dsg_queue_job_info()
        self.lib.check(self.lib.cdll.dsg_queue_job(self._q(), int(ticket), C.byref(info)))
        d = _JobInfo({k: int(getattr(info, k)) for k in ("state", "windows_done", "rows_ready", "slot", "first_round")})
        more = {"parks": int(info.reserved[2]), "held": bool(info.reserved[1] & L.JOB_HELD), "priority": self._prio[int(ticket)]}
        d.update({k: v for k, v in more.items() if v != _JobInfo.DEFAULTS[k]})
        if info.reserved[1] & L.JOB_LIVE:
            d.update(windows_given=int(info.reserved[0]), live=True, finished=bool(info.reserved[1] & L.JOB_FINISHED))
        return d

    def info(self) -> dict:
        r, p, n = C.c_int64(0), C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.cdll.dsg_queue_info(self._q(), C.byref(r), C.byref(p), C.byref(n)))
        return {"rounds_total": int(r.value), "n_pending": int(p.value), "n_running": int(n.value)}

    def rows(self, ticket):
        """The [rows_ready, J] view of the clip's result: the rows that are final so far."""
        return self._outs[int(ticket)][:self.job(ticket)["rows_ready"]]

    def result(self, ticket):
        """The whole clip [n_out, J]; raises unless the job is done.  A live clip: n_out of the windows it was given."""
        j = self.job(ticket)
        if j["state"] != L.JOB_DONE:
            raise L.DSGError(f"ClipQueue.result: ticket {int(ticket)} is not done (state {j['state']})")
        out = self._outs[int(ticket)]
        return out[:j["rows_ready"]] if j.get("live") else out

    def cancel(self, ticket):
        self.lib.check(self.lib.cdll.dsg_queue_cancel(self._q(), int(ticket)))
        self._keep.pop(int(ticket), None)

    def close(self):
        if self._handle is None:
            return
        q, self._handle = self._handle, None
        self.lib.check(self.lib.cdll.dsg_queue_close(q))
        self._keep.clear()
        self.diffusion._draw += self._advance


def _inpaint_mask(mask):
    """y['inpainting_mask'] as booleans (the reference negates it with `~`: a bool tensor); any non-zero entry of another dtype counts as set."""
    if L.is_torch(mask):
        import torch
        return mask if mask.dtype == torch.bool else mask != 0
    a = np.asarray(mask)
    return a if a.dtype == np.bool_ else a != 0


def create_gaussian_diffusion(timestep_respacing="", steps=1000, noise_schedule="cosine", library=None):
    """`create_gaussian_diffusion()` of main/utils/model_util.py:59-100 (cosine, 1000 steps, predict x_start,
    FIXED_SMALL, no respacing); `timestep_respacing="ddim50"` gives the DDIM-50 sampler of BASELINE config 3."""
    betas = get_named_beta_schedule(noise_schedule, steps, 1.)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return DSGDiffusion(space_timesteps(steps, timestep_respacing), betas, library=library)
