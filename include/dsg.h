/* dsg.h -- C ABI of libdsg_hip.so: the MI355X-native DDPM/DDIM sampling path of DiffuseStyleGesture.
 *
 * The reference (YoungSeng/DiffuseStyleGesture) is pure Python on PyTorch; it has no FFI for this path.  The
 * plugin surface it exposes is two Python call signatures, and every entry point below names the reference
 * interface it stands in for (paths relative to /root/reference):
 *
 *   dsg_create / dsg_load_tensor / dsg_finalize_weights
 *        MDM.__init__ + load_model_wo_clip(model, state_dict)       main/model/mdm.py:10-151, main/utils/model_util.py:8-12
 *        (tensor names = the checkpoint's state_dict keys)
 *   dsg_set_schedule
 *        SpacedDiffusion(use_timesteps, betas=...)                   main/diffusion/respace.py:73-87,
 *        GaussianDiffusion.__init__ tables                           main/diffusion/gaussian_diffusion.py:161-198
 *   dsg_set_window_cond
 *        the `y` dict of model_kwargs (style, seed, audio, mask_local) main/mydiffusion_zeggs/sample.py:227-251
 *   dsg_set_seed_last
 *        y['seed_last'] of DiffuseStyleGesture++ (cross_local_attention5)   BEAT-TWH-main/model/mdm.py:226-230,
 *                                                                    BEAT-TWH-main/mydiffusion_beat_twh/sample.py:85-93
 *   dsg_forward
 *        MDM.forward(x, timesteps, y)                                main/model/mdm.py:166-358
 *                                                                    BEAT-TWH-main/model/mdm.py:134-267
 *   dsg_sample
 *        GaussianDiffusion.p_sample_loop / ddim_sample_loop          main/diffusion/gaussian_diffusion.py:608-671, :889-936
 *   dsg_set_window_cond_cfg
 *        ClassifierFreeSampleModel.forward (y['scale'], y['uncond'])   main/model/cfg_sampler.py:8-31
 *   dsg_set_inpainting
 *        y['inpainting_mask'] / y['inpainted_motion'] in p_mean_variance   main/diffusion/gaussian_diffusion.py:317-321
 *   dsg_sample_clip / dsg_sample_clip_multi
 *        the window loop of inference(): seed hand-off, root shift,  main/mydiffusion_zeggs/sample.py:236-296,
 *        one-frame blend, stitching                                  BEAT-TWH-main/mydiffusion_beat_twh/sample.py:98-192
 *   dsg_set_clip_inpainting
 *        y['inpainting_mask'] / y['inpainted_motion'] of every window of that loop, given once in the stitched clip's frame
 *        coordinates and cut per window on the device                main/diffusion/gaussian_diffusion.py:317-321
 *   dsg_set_clip_init
 *        init_image (+ skip_timesteps) of every window of that loop, given once as a clip in the stitched clip's frame
 *        coordinates: x_t = q_sample(init_image, t, noise)            main/diffusion/gaussian_diffusion.py:701-713
 *   dsg_clone / dsg_sample_multi / dsg_set_kernel_set / dsg_get_kernel_set / dsg_recommend_kernel_set / dsg_last_kernel_set
 *        (no reference counterpart: the reference samples one clip at a time, sample.py:418 batch_size = 1; these run
 *         several clips of one GPU concurrently over one copy of the weights -- BASELINE config[3] "one clip per stream")
 *   dsg_noise
 *        th.randn(*shape) / th.randn_like(x)                         main/diffusion/gaussian_diffusion.py:704, :542
 *   dsg_pose2bvh
 *        pose2bvh(poses, outpath, length, smoothing)                 main/process/process_zeggs_bvh.py:219-275
 *   dsg_q_sample / dsg_predict_xstart_from_eps / dsg_posterior_step / dsg_ddim_step
 *        q_sample :236-254, _predict_xstart_from_eps :400-405, q_posterior_mean_variance + p_sample :256-278/:542-557,
 *        ddim_sample :773-792   (same file)
 *
 * Conventions: every function returns 0 on success or a negative DSG_E_* code; the message is available from
 * dsg_last_error() (thread local).  No C++ exception crosses this boundary.  Pointers may be host or device
 * pointers (detected with hipPointerGetAttributes); tensors are contiguous fp32 in the reference's layouts
 * ([B, J, 1, T] for poses/noise, frames fastest).  A handle is bound to one device and is not thread safe;
 * distinct handles are independent.  All work is enqueued on the handle's own stream and ordered after/before
 * the optional caller stream (`stream`, a hipStream_t) with events.
 */
#ifndef DSG_H_
#define DSG_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSG_VERSION 330

enum {
    DSG_OK = 0,
    DSG_E_INVALID = -1,       /* ValueError in the shim */
    DSG_E_RUNTIME = -2,       /* HIP runtime failure -> RuntimeError */
    DSG_E_UNEXPECTED_KEY = -3,/* load_model_wo_clip: unexpected state_dict key */
    DSG_E_MISSING_KEY = -4,   /* load_model_wo_clip: missing key at finalize */
    DSG_E_NOT_IMPLEMENTED = -5,
    DSG_E_STATE = -6          /* call order (e.g. sample before finalize / set_window_cond) */
};

/* DSG_PREC_BF16W2 (ABI 320): bf16 activations, every weight as hi + lo bf16 (16 mantissa bits), two MFMAs per weight fragment --
 * the precision mode between bf16 and fp32 (the bf16 drift of a 1000-step chain is the weights' 8-bit mantissa).  Kernel sets
 * LATENCY and TILE (every batch size) and, at latent_dim 128 / 256 without fused guidance, ROWS (round 6: k_clip_attn + the feed-forward kernel on
 * two-register fragments; DSG_KSET_AUTO picks it from 800 token rows -- 16 clips in lock step 453 -> 331 us per step) and, at the DSG+ widths
 * (latent_dim 384 / 512, 4 heads, ff 1024) without fused guidance, ROWS by name only (the QKV GEMM + k_attn + the feed-forward kernel on one 16-row tile,
 * 3 + 3L dispatches; DSG_KSET_AUTO stays on TILE there); BLOCK / STREAM are
 * DSG_E_NOT_IMPLEMENTED.  The reference computes in fp32
 * (main/train/training_loop.py:39: no autocast): DSG_PREC_FP32 is its arithmetic, the other two trade accuracy for speed. */
enum { DSG_PREC_FP32 = 0, DSG_PREC_BF16 = 1, DSG_PREC_BF16W2 = 2 };
/* kernel sets (dsg_set_kernel_set): which hand-written kernels one denoising step is made of.  Same arithmetic, different
 * grouping / tiling, i.e. last-bit differences between sets in bf16 -- which is why the set is an explicit, sticky property of
 * a handle and never depends on how a call is issued. */
enum {
    DSG_KSET_AUTO = 0,      /* by batch: LATENCY for batch <= 2 (latent_dim <= 256; the wider DSG+ models run TILE there), TILE below 1000
                               token rows, BLOCK from there, STREAM from 2000 */
    DSG_KSET_LATENCY = 1,   /* fused redundant-compute kernels, 2 + 3L dispatches: one clip in flight */
    DSG_KSET_TILE = 2,      /* one 16 x 16 MFMA tile per wave: small batches */
    DSG_KSET_BLOCK = 3,     /* 32-row block GEMMs + fused attention/out_proj/LayerNorm: large batches, several lanes.  ABI 320 (bf16, ZEGGS / tiny
                               widths): per layer k_clip_attn (per (clip, head): Q / K / V slices in LDS + attention) + the feed-forward half split
                               over ff with out_proj + LayerNorm1 as its prologue + the slab sum / LayerNorm2 pass: 3 + 3L dispatches; the DSG+
                               widths and fp32 get the ff-split behind k_attn_op_w */
    DSG_KSET_STREAM = 4,    /* weight-stationary persistent GEMMs (32x32x16 MFMA, global->LDS staging, 64-row blocks) for the pose
                               embedding and the pose head; per layer k_clip_attn + ONE feed-forward kernel (out_proj + LayerNorm1 as its
                               prologue, linear1 + GELU + linear2 + residual + LayerNorm2; ABI 320: 3 + 2L dispatches per step): >= 2000
                               token rows (23 ZEGGS clips) in one lane, >= 850 rows (10 clips) per lane with several lanes.  bf16, latent_dim 128 / 256, 4 heads -- the ZEGGS model;
                               DSG_E_NOT_IMPLEMENTED elsewhere */
    DSG_KSET_ROWS = 5       /* ABI 330: BLOCK's pose embedding / local attention / pose head around STREAM's per-layer pair, the feed-forward kernel on
                               ONE 16-row tile per workgroup (no ff-split, no partial slabs, no slab-sum pass: 3 + 2L dispatches).  Every workgroup
                               streams a layer's W_o + W1 + W2 for its 16 rows: it pays while the row tiles of all lanes fit the 256 CUs in one
                               round -- 800 .. 4096 token rows in one lane (9 .. 46 ZEGGS clips), fewer per lane with several lanes.  Same shapes
                               as STREAM, in bf16 and (without fused guidance) bf16w2.  At the DSG+ widths (bf16, latent_dim 384 / 512, 4 heads, ff 1024;
                               with fused guidance as well: the guided streaming pose head k_ws_cfg reads the conditional rows and their twins --
                               DSG_KSET_AUTO keeps guided calls on BLOCK, the set is reached by naming it): streamed pose embedding, then per layer the attention half per (clip, head) (k_clip_attn_w: the rows pass
                               through the LDS in chunks) + the same feed-forward kernel -- on 32-row blocks when >= 3 lanes together exceed one round of the
                               CUs -- = 3 + 2L dispatches; from
                               9 BEAT / 13 TWH clips in one lane, 4 per lane and 16 in all with several lanes.  bf16w2 at the DSG+ widths (no fused
                               guidance; by name only, DSG_KSET_AUTO keeps TILE): 16 x 16 tile pose embedding and pose head, per layer the QKV GEMM on the
                               hi + lo rows + k_attn + the feed-forward kernel on 16-row tiles = 3 + 3L dispatches.  DSG_E_NOT_IMPLEMENTED elsewhere */
};
enum { DSG_MODE_DDPM = 0, DSG_MODE_DDIM = 1 };

typedef struct dsg_config {
    int32_t variant;        /* 3 = cross_local_attention3_style1 (ZEGGS), 4 = cross_local_attention4 (BEAT/TWH) */
    int32_t njoints;        /* J */
    int32_t n_poses;        /* T, frames per window (multiple of `window`) */
    int32_t n_seed;         /* S */
    int32_t latent_dim;     /* D (multiple of 64, <= 512) */
    int32_t audio_src_dim;  /* A_src */
    int32_t audio_dim;      /* A */
    int32_t style_dim_in;
    int32_t window;         /* local attention window (<= 16) */
    int32_t num_layers;
    int32_t num_heads;      /* self-attention heads; head dim in {32, 64, 96, 128} */
    int32_t ff_size;
    int32_t local_heads;    /* 8 in the reference; head dim <= 64 */
    int32_t pe_max_len;     /* rows of sequence_pos_encoder.pe (5000) */
    int32_t train_steps;    /* rows of the time-embedding table = original diffusion steps (1000) */
    int32_t max_batch;
    int32_t precision;      /* DSG_PREC_* */
    int32_t device;         /* HIP device ordinal */
    int32_t steps_per_graph;/* > 0: denoising steps captured per hipGraph replay; 0 = default (eager: measured faster), -1 = eager */
    int32_t latency_mode;   /* DSG_KSET_AUTO only: 0 = by batch, 1 = never the LATENCY set, 2 = always (where AUTO can pick it at all:
                               latent_dim <= 256; dsg_recommend_kernel_set and the handle itself apply the same rule) */
    int32_t reserved[4];
} dsg_config;

typedef struct dsg_handle dsg_handle;

int dsg_version(void);
const char* dsg_last_error(void);

int dsg_create(const dsg_config* cfg, dsg_handle** out);
/* a further sampling lane over the SAME weights (reference counted; call after dsg_finalize_weights): own stream / HSA queue,
 * state, conditioning and schedule.  max_batch <= 0: the source's.  One lane per concurrently sampled clip ("one clip per
 * stream", BASELINE config[3]); see dsg_sample_multi.  Reloading weights into the source does not update existing clones. */
int dsg_clone(dsg_handle* src, int max_batch, dsg_handle** out);
int dsg_destroy(dsg_handle* h);

/* dtype: 0 = float32.  shape/ndim are checked against the model dims. */
int dsg_load_tensor(dsg_handle* h, const char* name, const void* data, const int64_t* shape, int ndim, int dtype);
/* repack weights into MFMA fragment order (bf16 or fp32), fold input_process2 . poseEmbedding, build the
 * [train_steps, D] time-embedding tables and rotary tables */
int dsg_finalize_weights(dsg_handle* h);
/* betas: the (respaced) beta schedule, float64[n]; timestep_map: original timestep of each kept step, int64[n] */
int dsg_set_schedule(dsg_handle* h, const double* betas, const int64_t* timestep_map, int n);
/* host-only helper (no device needed): the 11 float64[n] tables of GaussianDiffusion.__init__, written to
 * out[11*n] in the order betas, alphas_cumprod, alphas_cumprod_prev, sqrt_alphas_cumprod,
 * sqrt_one_minus_alphas_cumprod, sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_variance,
 * posterior_log_variance_clipped, posterior_mean_coef1, posterior_mean_coef2 */
int dsg_schedule_tables(const double* betas, int n, double* out);

/* variant 5 only: seed_last [B, J, 1, S]; kept until replaced; must precede dsg_set_window_cond with the same B */
int dsg_set_seed_last(dsg_handle* h, const float* seed_last, int B, void* stream);

/* style [B, style_dim_in]; seed [B, J, 1, S]; audio [B, T_a, A_src] (T_a = T for variant 3, T-S for variant 4, T-2S for 5);
 * mask_local uint8 [mask_batch, T] (1 = keep), mask_batch in {1, B}; NULL = the reference's `mask=None` (nothing masked but
 * the causal future: the look-back pad keys of window 0 attend with value -1, local_attention.py:196);
 * uncond != 0 -> uncond_info / y['uncond'].  The caller's buffers may be reused once `stream` has passed this call. */
int dsg_set_window_cond(dsg_handle* h, const float* style, const float* seed, const float* audio,
                        const uint8_t* mask_local, int mask_batch, int B, int uncond, void* stream);
/* classifier-free guidance, ClassifierFreeSampleModel.forward (main/model/cfg_sampler.py:8-31) fused into the path: the
 * B elements and their unconditional twins (y['uncond'] = True) run as ONE batch of 2B rows (max_batch >= 2B) and the
 * pose-head epilogue forms out_uncond + scale[b] * (out - out_uncond) before the sampler update.  scale: float[B]
 * (y['scale']).  dsg_forward / dsg_sample are then called with the user batch B as usual. */
int dsg_set_window_cond_cfg(dsg_handle* h, const float* style, const float* seed, const float* audio,
                            const uint8_t* mask_local, int mask_batch, int B, const float* scale, void* stream);

/* Motion inpainting, p_mean_variance with y['inpainting_mask'] and y['inpainted_motion'] (main/diffusion/gaussian_diffusion.py:317-321):
 * mask uint8 [B, J, 1, T] (non-zero = keep the given motion), motion fp32 [B, J, 1, T], host or device.  Every step of dsg_sample /
 * dsg_sample_multi then sets x0 = mask ? motion : x0 -- after the guidance combination (the model is the ClassifierFreeSampleModel), before
 * clip_denoised and the posterior / DDIM update -- inside the pose-head epilogue; dsg_forward is not affected (MDM.forward does not inpaint).
 * Sticky for the handle: dsg_set_window_cond* leaves it alone, dsg_sample needs the same B.  mask == NULL && motion == NULL switches it off
 * (B ignored); exactly one NULL, or B > max_batch: DSG_E_INVALID.  A dsg_clone starts without a constraint; every lane of dsg_sample_multi
 * has its own.  With const_noise only the noise is shared, not the constraint.  Added without a version step: one more export changes no
 * existing layout or call, dsg_version() stays 330. */
int dsg_set_inpainting(dsg_handle* h, const uint8_t* mask, const float* motion, int B, void* stream);

/* x, out: [B, J, 1, T] fp32; t: model timesteps int64[B] (each < train_steps) */
int dsg_forward(dsg_handle* h, const float* x, const int64_t* t, float* out, int B, void* stream);

typedef struct dsg_sample_args {
    int32_t mode;             /* DSG_MODE_DDPM / DSG_MODE_DDIM */
    int32_t skip_timesteps;
    float eta;                /* DDIM only */
    int32_t const_noise;      /* p_sample(const_noise=True): batch element 0's noise for everyone */
    const float* init_noise;  /* nullable [B,J,1,T]: the reference's `noise=` argument (x_T) */
    const float* step_noise;  /* nullable [n_run,B,J,1,T]: replayed per-step noise; else the Philox stream */
    const float* init_image;  /* nullable [B,J,1,T] */
    uint64_t seed;            /* Philox key */
    uint64_t stream_id;       /* Philox stream (e.g. clip index) */
    uint32_t draw_base;       /* draw index of x_T; step i uses draw_base + 1 + i */
    int32_t n_dump;           /* dump_steps support: number of entries in dump_steps */
    const int32_t* dump_steps;/* host int32[n_dump], ascending loop indices */
    float* dump_out;          /* [n_dump,B,J,1,T] */
    int32_t clip_denoised;    /* != 0: x0 clamped to [-1, 1] before the update (clip_denoised=True, gaussian_diffusion.py:377-379) */
    int32_t first_step;       /* ABI 310: run the chain in pieces (the lazy p_sample_loop_progressive, gaussian_diffusion.py:673-740): loop */
    int32_t max_steps;        /* index this call starts at (> 0: init_noise is x_t of that step, taken as it is) and how many steps it runs */
    int32_t reserved[1];      /* (0 = to the end); draw indices, dump_steps and step_noise stay those of the whole chain */
} dsg_sample_args;

/* runs num_timesteps - skip_timesteps denoising steps for the conditioning set by dsg_set_window_cond;
 * out [B,J,1,T] receives the final sample.  With the default AQL submission of the step loop (csrc/dsg_aql.h) the call
 * returns when the steps have run; with HIP launches (DSG_AQL=0, or under a profiler) it only enqueues and is asynchronous
 * w.r.t. the host when `out` is device memory. */
int dsg_sample(dsg_handle* h, const dsg_sample_args* args, float* out, int B, void* stream);
/* n lanes (a handle and its dsg_clone()s: one device, shared weights; n <= 16), one independent sampling call each, run
 * concurrently from this one host thread -- "one clip per stream": every lane owns an HSA queue, the dependent packet chains
 * of the lanes overlap on the GPU.  args[n], outs[n]; every lane samples a batch of B.  Every lane runs the kernel set of ITS
 * handle, so lane i's result is bit-identical to dsg_sample(lanes[i], &args[i], outs[i], B, stream) issued on its own. */
int dsg_sample_multi(dsg_handle** lanes, int n, const dsg_sample_args* args, float** outs, int B, void* stream);
/* A whole clip in one call: the K windows of the reference's inference() loops (main/mydiffusion_zeggs/sample.py:236-296,
 * BEAT-TWH-main/mydiffusion_beat_twh/sample.py:98-192) for B clips in lock step.  Per window the library sets the conditioning
 * (as dsg_set_window_cond / _cfg: `scale` float[B] or NULL), runs the step loop exactly as dsg_sample does, and hands the window
 * over on the device (k_window_handoff): window c > 0 is shifted so that its root position (features 0..2) continues the previous
 * window's when root_shift != 0 (sample.py:277-281), its frame 0 is blended half and half with the previous window's frame T - S
 * (the reference's `len(last_poses) == 1` quirk), frames [0, T - S) are appended to the clip, and its last S frames are window
 * c + 1's y['seed'].  style [B, style_dim_in]; seed0 [B, J, 1, S] = y['seed'] of window 0, NULL = zeros (sample.py:241);
 * audio [K, B, T_a, A_src] = the K per-window features exactly as dsg_set_window_cond takes them (variant 3 of the BEAT-TWH tree:
 * the caller prepends the left context, as before); mask_local / mask_batch as dsg_set_window_cond, the same for every window.
 * out [B, n_out, J] fp32, host or device, frame-major (NOT [B, J, 1, T]): keep_last_tail == 0 (ZEGGS) cuts the last overlap and
 * the first S frames, n_out = K * (T - S) - S; keep_last_tail != 0 (DSG+) keeps the last window whole, n_out = K * (T - S).
 * args: as dsg_sample; draw_base is window 0's, window c draws from draw_base + c * (1 + n_run) -- what K consecutive dsg_sample
 * calls consume -- so the result is bit-identical to those K calls + the stitching of sample.py under the same kernel set.
 * DSG_E_INVALID: K < 1; a handle with a window-level inpainting constraint (dsg_set_inpainting is per window; a whole clip takes
 * dsg_set_clip_inpainting, below); step_noise, init_noise, init_image, n_dump, first_step or max_steps in args (per-window tensors /
 * pieces of one chain; a whole clip to start from takes dsg_set_clip_init, below).  Variant 5 needs dsg_set_seed_last first.
 * dsg_last_sample_ms afterwards: the sum over the K step loops, n_steps their total.  _multi: n lanes as dsg_sample_multi, one clip
 * batch each (styles[n], audios[n], outs[n], args[n]; seed0s / scales: NULL or n entries, each nullable), the windows advance in
 * lock step over the lanes.  Added without a version step, as dsg_set_inpainting: dsg_version() stays 330. */
int dsg_sample_clip(dsg_handle* h, const float* style, const float* seed0, const float* audio, const uint8_t* mask_local,
                    int mask_batch, const float* scale, const dsg_sample_args* args, int K, int root_shift, int keep_last_tail,
                    float* out, int B, void* stream);
int dsg_sample_clip_multi(dsg_handle** lanes, int n, const float* const* styles, const float* const* seed0s,
                          const float* const* audios, const uint8_t* mask_local, int mask_batch, const float* const* scales,
                          const dsg_sample_args* args, int K, int root_shift, int keep_last_tail, float** outs, int B, void* stream);
/* Clip queue: clips of DIFFERENT lengths share one batch of slots.  dsg_sample_clip / _multi advance B clips in lock step, so every clip of
 * a call has the same number of windows K; a corpus of recordings from seconds to minutes then either runs in groups padded to each group's
 * longest clip or one clip at a time.  The queue gives every clip (a job) a slot of the n_lanes * B slots and refills a slot when its clip
 * ends.  Every clip comes out bit for bit as dsg_sample_clip produces it alone -- B = 1, args->seed = job.seed, args->stream_id =
 * job.stream_id, the same draw_base, conditioning, root_shift / keep_last_tail -- under the same named kernel set: its noise is keyed by its
 * own Philox pair (as dsg_set_noise_streams keys a batch), a slot on window c of its clip draws draw_base + c * (1 + n_run) for x_T and the
 * following n_run for the steps (a per-element draw offset read beside the element's key), and the hand-off (root shift, one-frame blend,
 * stitching, next seed: k_window_handoff_q) knows each slot's clip.  Reference counterpart: none -- the reference samples one clip at a
 * time (main/mydiffusion_zeggs/sample.py:418).
 * A job: style [style_dim_in]; seed0 [J, 1, S] = y['seed'] of window 0 (NULL: zeros); seed_last [J, 1, S] (variant 5: required, else NULL);
 * audio [K, T_a, A_src] = the clip's K per-window features as dsg_sample_clip takes them; out [n_out(K), J] with n_out(K) = K * (T - S) - S,
 * or K * (T - S) with keep_last_tail; scale = y['scale'], read when guided != 0; (seed, stream_id) = the clip's Philox pair.  Every pointer
 * host or device.  A device `out` is written by the hand-off itself; host ones go through one library-owned device buffer, one copy per job.
 * The plan (dsg_clip_queue_plan: host only, no device, and exactly what the queue call follows): jobs are taken longest first (K descending,
 * ties by lower index); each goes to the slot with the least load so far (ties: lowest slot); first_round[j] is that load, slot[j] the slot,
 * *n_rounds the largest load.  Global slot s of n_slots = n_lanes * B is lane s % n_lanes, position s / n_lanes.  The call runs n_rounds
 * rounds; a round is one window of dsg_sample_clip_multi for every lane at the constant batch B (with guided != 0: B conditional elements +
 * their B twins).  A slot without a clip in a round -- finished, or never given one -- keeps running on the conditioning it holds and writes
 * nothing; rows are independent, so nothing of it reaches a clip.  mask_local: uint8[T] shared by every slot, or NULL.  args: mode,
 * skip_timesteps, eta, clip_denoised and draw_base are read (draw_base is every clip's); seed / stream_id are ignored.  Each lane runs the
 * kernel set of ITS handle (DSG_KSET_AUTO: by B, as ever).  dsg_last_sample_ms afterwards: the sum over the rounds, n_steps = n_rounds * n_run.
 * DSG_E_INVALID, each with the cause in dsg_last_error: n_jobs < 1; a job with K < 1, a null style / audio / out, or (variant 5) no
 * seed_last; B < 1 or B (2 B with guided) > max_batch; n_lanes > 16; lanes of different models, devices or step counts; args with
 * step_noise, init_noise, init_image, n_dump, first_step, max_steps or const_noise; a handle that carries sticky noise streams
 * (dsg_set_noise_streams), a window-level or clip-level inpainting constraint, or a clip-level init motion -- the handle-level setters are
 * [B, n_frames, J] for one n_frames; in a queue the constraint and the init motion travel with the job (dsg_sample_clip_queue_edit below).
 * DSG_E_STATE: before dsg_finalize_weights / dsg_set_schedule.
 * On every return path, errors included, the lanes are left as they came: unkeyed, no draw offsets, one lane.  Variant 5: the call overwrites
 * the lanes' y['seed_last'] rows, so a later dsg_set_window_cond needs dsg_set_seed_last again.
 * Added without a version step, as the setters above: dsg_version() stays 330. */
typedef struct dsg_clip_job {
    const float* style;      /* [style_dim_in] */
    const float* seed0;      /* [J,1,S] = y['seed'] of window 0; NULL = zeros */
    const float* seed_last;  /* variant 5: [J,1,S]; NULL otherwise */
    const float* audio;      /* [K, T_a, A_src], the K per-window features as dsg_sample_clip takes them */
    float* out;              /* [n_out(K), J]; n_out(K) = K*(T-S)-S, or K*(T-S) with keep_last_tail */
    int32_t K;               /* >= 1 */
    float scale;             /* y['scale'], read when guided != 0 */
    uint64_t seed, stream_id;/* the clip's Philox pair */
    int32_t reserved[4];
} dsg_clip_job;
int dsg_clip_queue_plan(const int32_t* K, int n_jobs, int n_slots, int32_t* slot, int32_t* first_round, int32_t* n_rounds);
int dsg_sample_clip_queue(dsg_handle** lanes, int n_lanes, const dsg_clip_job* jobs, int n_jobs, int B, const uint8_t* mask_local, int guided,
                          const dsg_sample_args* args, int root_shift, int keep_last_tail, void* stream);
/* Motion inpainting over a whole clip, for dsg_sample_clip / _multi: mask uint8 [B, n_frames, J] (non-zero = keep the given motion), motion
 * fp32 [B, n_frames, J]; host or device; frame-major, exactly the layout and frame numbering of dsg_sample_clip's `out`.  Sticky for the
 * handle, like dsg_set_inpainting.  The library keeps its own device copy (allocated on first use, grown when needed, freed with the
 * handle): the caller's buffers are free once `stream` has passed the call.  mask == NULL && motion == NULL switches it off (B, n_frames
 * ignored); exactly one NULL, B > max_batch or n_frames < 1: DSG_E_INVALID.  A dsg_clone starts without a constraint; every lane of
 * dsg_sample_clip_multi has its own, lanes without one run as before.  dsg_forward, dsg_sample and dsg_sample_multi ignore it.
 * dsg_sample_clip / _multi on a handle that carries it need the same B and n_frames == n_out (K * (T - S) - S without keep_last_tail,
 * K * (T - S) with it), else DSG_E_INVALID with both numbers in the message; a window-level constraint (dsg_set_inpainting) on the handle
 * is refused by them as before.
 * Semantics, keep = T - S: frame f of window c is clip row df = c * keep + f - S.  For 0 <= df < n_out the window's constraint at (b, j, f)
 * is the clip's at (b, df, j); elsewhere -- the first S frames of window 0, the closing S frames of the last window when they are cut -- the
 * frame is unconstrained.  The tail of window c (f >= keep) therefore carries the constraint of the rows window c + 1 will write: the seed
 * it hands over honours it already.  The constraint acts where the window-level one does: after the guidance combination, before
 * clip_denoised and the update.  Between two step loops the library cuts the next window's slice on the device (k_clip_inp_window); the
 * result is bit-identical to K dsg_sample calls, each after dsg_set_inpainting with that window's slice, + the stitching of sample.py,
 * under the same kernel set and the same draws.
 * Root shift: with root_shift != 0 the three root-position channels (features 0..2) of windows c > 0 are constrained in the window's own
 * frame, that is BEFORE the shift -- which is what the K-call sequence does; the stitched clip then holds the constrained value moved by
 * the window's delta.  A caller who pins the root trajectory passes root_shift = 0.  Hand-off frames: when both sides of a hand-off frame
 * (frame T - S of window c, frame 0 of window c + 1: one clip row) are constrained, they are constrained to the same value; the
 * half-and-half blend then returns that value exactly, and the shift delta of a constrained root channel there is 0.
 * Added without a version step, as dsg_set_inpainting: dsg_version() stays 330. */
int dsg_set_clip_inpainting(dsg_handle* h, const uint8_t* mask, const float* motion, int B, int n_frames, void* stream);
/* Editing an existing clip, for dsg_sample_clip / _multi: the motion every window is re-denoised from -- init_image + skip_timesteps of
 * p_sample_loop (main/diffusion/gaussian_diffusion.py:701-713, x_t = q_sample(init_image, t, noise)) for the whole window loop.  motion fp32
 * [B, n_frames, J], host or device; frame-major, exactly the layout and frame numbering of dsg_sample_clip's `out`.  Sticky for the handle.
 * The library keeps its own device copy (allocated on first use, grown when needed, freed with the handle): the caller's buffer is free
 * once `stream` has passed the call.  motion == NULL switches it off (B, n_frames ignored); B > max_batch or n_frames < 1: DSG_E_INVALID.
 * A dsg_clone starts without one; every lane of dsg_sample_clip_multi has its own, lanes without one run as before.  dsg_forward,
 * dsg_sample and dsg_sample_multi ignore it.
 * dsg_sample_clip / _multi on a handle that carries it need the same B and n_frames == n_out, else DSG_E_INVALID with both numbers in the
 * message.  Window c then starts from q_sample(slice_c, t_start, noise) with t_start = the first timestep the call runs (skip_timesteps
 * == 0 is allowed: the last timestep, as in the reference) and noise = draw draw_base + c * (1 + n_run) -- the draw K dsg_sample calls
 * with init_image would use; the draw accounting is unchanged.  args.init_image / init_noise stay refused.  It combines with
 * dsg_set_clip_inpainting, with guidance (the unconditional twins receive the same start) and with DDIM.
 * The slice, keep = T - S: frame f of window c is clip row df = c * keep + f - S; for 0 <= df < n_frames the init value at (b, j, f) is
 * the clip's at (b, df, j).  Rows outside the clip:
 *   df < 0          (window 0, frames f < S: the frames the seed poses stand for in training)  y['seed'] of window 0 at (b, j, f) -- the
 *                   caller's seed0, or the zeros the call puts there without one;
 *   df >= n_frames  (the closing S frames of the last window, without keep_last_tail only)     clip row n_frames - 1, a held pose.
 * The cut, q_sample and the write of the sampler state are one kernel (k_clip_x_in) per window; the result is bit-identical to K dsg_sample
 * calls, each with init_image = that window's slice as [B, J, 1, T], + the stitching of sample.py, under the same kernel set and draws.
 * Root shift: with root_shift != 0 the slice is taken in the window's own frame, that is BEFORE the shift -- which is what the K-call
 * sequence does: windows c > 0 start from the given root trajectory and the hand-off then moves them by the window's delta.
 * Added without a version step, as the two inpainting setters: dsg_version() stays 330. */
int dsg_set_clip_init(dsg_handle* h, const float* motion, int B, int n_frames, void* stream);
/* Clip queue with per-clip edits: dsg_sample_clip_queue where every job may bring its own inpainting constraint and / or the clip it is
 * re-denoised from.  edits: NULL, or one dsg_clip_edit per job, parallel to jobs[]; dsg_sample_clip_queue(...) IS this call with edits ==
 * NULL (same bits, same launches).  The three tensors of an edit are [n_out(K), J] in the layout and frame numbering of the job's `out`
 * -- exactly what dsg_set_clip_inpainting / dsg_set_clip_init take for one batch element -- each host or device memory, each nullable.
 * Job j comes out bit for bit as dsg_sample_clip produces it alone: B = 1, the job's (seed, stream_id), the same draw_base, conditioning,
 * root_shift / keep_last_tail and named kernel set, after dsg_set_clip_inpainting(h, inp_mask, inp_motion, 1, n_out) and / or
 * dsg_set_clip_init(h, init_motion, 1, n_out).  A job without edits beside jobs with some comes out as it does alone without edits: the
 * pose-head epilogue selects per mask byte, so a slot whose mask is all zero keeps its x0 bits.
 * Semantics per slot: those written above for the two setters, with the slot's own clip -- df = c * (T - S) + f - S; the constraint leaves
 * frames outside [0, n_out) free; the init takes window 0's y['seed'] of that slot for df < 0 and holds clip row n_out - 1 for df >= n_out;
 * root_shift is applied after either, in the window's own frame; guidance twins get the same start, the constraint acts after the
 * combination; skip_timesteps == 0 with an init is allowed (the last timestep).  In a call where some job has an init motion, a slot without
 * one starts exactly as it does in dsg_sample_clip_queue: q_sample of a zero init with skip_timesteps > 0, the draw itself with
 * skip_timesteps == 0 (skip_timesteps is the call's here; dsg_sample_clip_queue_steps below gives every job its own, so that fresh clips
 * and edits share one call).  A dead slot is a slot without edits.
 * On the device: per round one table of {constraint, init, n_out, c} per slot goes up beside the hand-off's; k_clipq_inp_window cuts every
 * slot's constraint into the buffers of dsg_set_inpainting (lanes that run a constrained job only; without any, no cut kernel runs), and
 * k_clipq_x_in starts the round in place of the plain start kernel (lanes that run a job with an init motion only).
 * Staging: device tensors are read where they are and must stay valid until `stream` has passed the call.  Host tensors are uploaded before
 * the first round, each on the stream of the lane that runs the job (slot[j] % n_lanes), into library-owned device memory of that lane
 * (grown when needed, freed with the handle) that holds ALL host-side edits of the call's jobs on that lane at once: 9 * n_out * J bytes for
 * a job with both edits (+ up to 15 bytes of padding per tensor).
 * DSG_E_INVALID, with the cause and the job number in dsg_last_error: exactly one of inp_mask / inp_motion is NULL; and everything
 * dsg_sample_clip_queue refuses, handles that carry the sticky dsg_set_clip_inpainting / dsg_set_clip_init included.  On every return
 * path, errors included, the lanes are left as they came: no inpainting (dsg_set_inpainting's batch 0), no edit table, unkeyed, one lane.
 * dsg_clip_job keeps its layout; its `reserved` stays unread.  Added without a version step: dsg_version() stays 330. */
typedef struct dsg_clip_edit {      /* one per job, parallel to jobs[]; all three nullable */
    const uint8_t* inp_mask;        /* [n_out(K), J]  non-zero = keep inp_motion there           */
    const float*   inp_motion;      /* [n_out(K), J]                                             */
    const float*   init_motion;     /* [n_out(K), J]  the clip to re-denoise from                */
    int32_t reserved[2];
} dsg_clip_edit;
int dsg_sample_clip_queue_edit(dsg_handle** lanes, int n_lanes, const dsg_clip_job* jobs, const dsg_clip_edit* edits /* NULL or [n_jobs] */,
                               int n_jobs, int B, const uint8_t* mask_local, int guided, const dsg_sample_args* args,
                               int root_shift, int keep_last_tail, void* stream);
/* Clip queue with per-clip skip_timesteps: one queue for generate and edit requests.  skip_timesteps -- how deep a clip is noised before it is
 * sampled back, the strength of an edit -- travels with the job like its init motion and its constraint: skip_timesteps NULL, or int32
 * [n_jobs] parallel to jobs[]; an entry < 0 reads as args->skip_timesteps.  Fresh generations (skip 0, from pure noise) and edits of any depth
 * then share the slots of one call.  dsg_sample_clip_queue_edit(...) IS this call with skip_timesteps == NULL; with NULL, or with every entry
 * equal to the call's skip, the call makes the same launches and produces the same bits, and its plan is dsg_clip_queue_plan's.
 * Job j comes out bit for bit as dsg_sample_clip produces it alone with args->skip_timesteps = skip_j: B = 1, the job's (seed, stream_id),
 * the same draw_base, conditioning, root_shift / keep_last_tail, named kernel set and edits, DDPM and DDIM.  Everything written above for
 * dsg_sample_clip_queue_edit holds per slot with the slot's own skip: a slot with an init motion starts from q_sample of its slice at ITS
 * first timestep (skip 0 with an init is allowed: the last timestep), a slot without one from q_sample of a zero init when its skip is
 * > 0 and from the draw itself when it is 0; window c of job j draws draw_base + c * (1 + n_run_j) for its start and the following n_run_j
 * for its steps, n_run_j = num_timesteps - skip_j.
 * Rounds: with n = num_timesteps, round r runs ONE loop for all lanes from s_r = the smallest skip alive in it (over all lanes), n - s_r
 * steps, as dsg_sample does with skip_timesteps = s_r: loop index i is timestep index n - 1 - s_r - i for every element, so the time
 * embedding and the step coefficients stay one set per step.  A slot with skip_b > s_r HOLDS for its first skip_b - s_r loop indices: the
 * pose-head epilogue leaves the element alone -- no draw, no write of its state, its bf16 shadow or its guidance twin -- and its chain runs
 * on the loop's last n - skip_b steps, on the timesteps it runs alone.  A held element's rows still pass through the denoiser (rows are
 * independent: the argument that covers dead slots), so a light edit beside a fresh clip occupies its slot for the fresh clip's steps;
 * the plan keeps that small.  Per-element timesteps (slots on different timesteps within one step) are not part of this.
 * The plan (dsg_clip_queue_plan_steps: host only, exactly what the call follows; n_run[j] = n - skip_j, NULL: all equal): jobs are taken
 * deepest first (n_run descending, then K descending, then lower index); each goes to the slot with the fewest rounds so far (ties: lowest
 * slot); slot / first_round / n_rounds as dsg_clip_queue_plan; *total_steps (nullable) = the sum over the rounds of the largest n_run alive
 * in that round.  With n_run == NULL the order and outputs are dsg_clip_queue_plan's and total_steps = n_rounds.  The deep jobs go first, so
 * the closing rounds hold only light ones and run short.  Example: 24 fresh clips and 24 edits with n_run = 100, all K = 4, on 16 slots of
 * a 1000-step schedule: 8 rounds of 1000 steps and 4 rounds of 100, 8 400 steps in all; two separate calls take 8 800, index-order placement
 * of an interleaved job list up to 12 000.  The gain in steps is modest; the point is one queue for everything.
 * On the device: per slot one 8-byte word {draw offset, hold} beside the element's key (the offset is c * (1 + n_run_j) - hold: the
 * element's step i is the round's loop index i + hold); in a call with per-job skips every lane starts every round through k_clipq_x_in,
 * whose table carries per slot whether to q_sample and the fp32 pair sqrt(abar), sqrt(1 - abar) of the slot's own first timestep -- the
 * two values the stand-alone start kernels get for skip_timesteps = skip_b.
 * dsg_last_sample_ms afterwards: the sum over the rounds, n_steps = the sum over the rounds of n - s_r = the plan's total_steps.
 * DSG_E_INVALID, with the job number in dsg_last_error: a skip outside [0, n - 1] after the substitution; and everything
 * dsg_sample_clip_queue_edit refuses.  On every return path, errors included, the lanes are left as they came: no inpainting, no edit
 * table, unkeyed, no draw offsets and no holds, one lane.  dsg_clip_job and dsg_clip_edit keep their layouts.  Added without a version
 * step: dsg_version() stays 330. */
int dsg_sample_clip_queue_steps(dsg_handle** lanes, int n_lanes, const dsg_clip_job* jobs, const dsg_clip_edit* edits /* NULL or [n_jobs] */,
                                const int32_t* skip_timesteps /* NULL or [n_jobs]; an entry < 0: args->skip_timesteps */,
                                int n_jobs, int B, const uint8_t* mask_local, int guided, const dsg_sample_args* args,
                                int root_shift, int keep_last_tail, void* stream);
int dsg_clip_queue_plan_steps(const int32_t* K, const int32_t* n_run /* NULL: all equal */, int n_jobs, int n_slots,
                              int32_t* slot, int32_t* first_round, int32_t* n_rounds, int64_t* total_steps /* nullable */);
/* Clip queue as a session: submit while it runs, collect per window.  dsg_sample_clip_queue[_edit|_steps] take a closed list of jobs and
 * return when all of them are done; a session (dsg_queue) lives between rounds, so a request that arrives while others run takes the next free
 * slot, and a clip's rows are in the caller's memory after the round that made them final.  A round is a round of
 * dsg_sample_clip_queue_steps: it starts from the smallest skip alive, slots with a larger skip hold, dead slots run on the conditioning they
 * hold and write nothing, job j draws draw_base + c * (1 + n_run_j) for the start of its window c and the following n_run_j for its steps,
 * edits go through the per-round edit table.  The promise is the queue's: job j comes out bit for bit as dsg_sample_clip produces it alone
 * -- B = 1, its (seed, stream_id), its skip and edits, the same draw_base, root_shift / keep_last_tail and named kernel set -- whenever it was
 * submitted, whatever ran beside it, whatever was cancelled.  Reference counterpart: none.
 * dsg_queue_open: the checks of dsg_sample_clip_queue_steps on lanes, B, guided and args, with the same refusals and messages.  `guided` is
 * fixed for the session (it decides the batch layout); every job runs at its own `scale`.  args and mask_local (uint8[T], host or device, or
 * NULL) are copied.  From open to close the lanes belong to the session: dsg_sample*, dsg_forward, the dsg_set_* setters, dsg_load_tensor,
 * dsg_finalize_weights, dsg_destroy and a second dsg_queue_open on such a handle return DSG_E_STATE ("handle belongs to an open queue");
 * dsg_clone, dsg_sync, dsg_get_* and dsg_last_* stay usable.  Like a handle, a session is not thread safe: a service calls submit and run
 * from one thread, alternating.
 * dsg_queue_submit: the per-job checks of the queue calls; edit nullable; skip_timesteps < 0 reads as args->skip_timesteps.  *ticket counts
 * from 0 in submission order.  OWNERSHIP: host tensors of the job -- style, seed0, seed_last, the K audio windows, the three edit tensors --
 * are copied into session-owned device memory before the call returns, so the caller's host buffers are free on return.  Device tensors are
 * read where they are, behind whatever `stream` has enqueued, and must stay valid until the job is DONE or CANCELLED.  `out` stays the
 * caller's until then, host or device.  Staging blocks are recycled inside the session and released at close.  An allocation that fails:
 * DSG_E_RUNTIME, and the session is as it was.
 * PLACEMENT (with equal priorities; "Priorities, park and resume" below states the whole rule): at the start of every round the free slots take
 * the pending jobs -- lowest free slot first, oldest ticket first.  Global slot s is
 * lane s % n_lanes, position s / n_lanes, as in the one-shot call.  First come, first served is deliberate: predictable latency is what a
 * session is for.  A caller who holds the whole corpus submits it longest first, which reproduces the one-shot plan, or keeps using the
 * one-shot call.  dsg_queue_place is this rule on the host (no device): arrive_round[j] = the session round before which job j is submitted,
 * non-negative and non-decreasing, NULL = all 0; slot / first_round / n_rounds as dsg_clip_queue_plan.  DSG_E_INVALID: K < 1, n_jobs < 1,
 * n_slots < 1, decreasing arrivals.
 * dsg_queue_run: up to max_rounds rounds (<= 0: until idle); returns early, with *rounds_run (nullable) as counted, when nothing is alive
 * or pending.  On return rows [0, rows_ready) of every host `out` are in the caller's memory and final; rows past rows_ready are untouched.
 * rows_ready = min(n_out, windows_done * (T - S) - S), n_out when the job is done: window c leaves rows [c * (T - S) - S, (c + 1) * (T - S) - S)
 * final, with keep_last_tail as without -- there only the last window writes its closing S frames.
 * Device `out`s are written by the hand-off itself and ordered before `stream`.  dsg_last_sample_ms on a lane afterwards: the sum over the
 * rounds of this run call, n_steps their step total.  After an error from run the session is only good for dsg_queue_close.
 * dsg_queue_job / dsg_queue_info: the state of one ticket / of the session (every pointer of _info nullable).
 * dsg_queue_cancel: a pending job never runs; a running job's slot is dead from the next round on and the rows written so far stay; no
 * other job is affected; a job that is done or cancelled already: no-op.
 * dsg_queue_close: allowed with jobs pending or running, which are abandoned.  The lanes are left as the one-shot call leaves them on every
 * return path -- unkeyed, no draw offsets or holds, no inpainting, no edit table, one lane; variant 5 asks for dsg_set_seed_last again --
 * and the staging memory is freed.
 * On the device: per lane and round one table of {style, audio window c, seed0, seed_last, flags} per slot goes up beside the hand-off's and
 * k_clipq_gather copies the round's conditioning into the lane's buffers in one launch (the one-shot call issues up to 2 B copies per lane
 * from the caller's memory); every lane starts every round through k_clipq_x_in, as the one-shot call does with per-job skips.
 * Added without a version step: dsg_version() stays 330; dsg_clip_job and dsg_clip_edit keep their layouts. */
typedef struct dsg_queue dsg_queue;
enum { DSG_JOB_PENDING = 0, DSG_JOB_RUNNING = 1, DSG_JOB_DONE = 2, DSG_JOB_CANCELLED = 3 };
typedef struct dsg_queue_job_info {
    int32_t state;         /* DSG_JOB_*                                                   */
    int32_t windows_done;  /* windows handed off so far                                   */
    int32_t rows_ready;    /* rows [0, rows_ready) of the job's `out` are final and there */
    int32_t slot;          /* global slot, -1 while pending                               */
    int32_t first_round;   /* session round of its window 0, -1 while pending             */
    int32_t windows_given; /* a live job: the windows given so far; 0 for a closed job    */
    int32_t live;          /* DSG_JOB_LIVE | DSG_JOB_FINISHED | DSG_JOB_HELD; 0 for a closed job nobody holds */
    int32_t reserved[1];   /* [0]: parks -- how often the job has been parked (priorities, below); 0 for a job never parked */
} dsg_queue_job_info;
enum { DSG_JOB_LIVE = 1, DSG_JOB_FINISHED = 2 };      /* dsg_queue_job_info.live */
int dsg_queue_open(dsg_handle** lanes, int n_lanes, int B, const uint8_t* mask_local, int guided,
                   const dsg_sample_args* args, int root_shift, int keep_last_tail, dsg_queue** out);
int dsg_queue_submit(dsg_queue* q, const dsg_clip_job* job, const dsg_clip_edit* edit /* nullable */,
                     int skip_timesteps /* < 0: args->skip_timesteps */, int64_t* ticket, void* stream);
int dsg_queue_run(dsg_queue* q, int max_rounds /* <= 0: until idle */, int* rounds_run, void* stream);
int dsg_queue_job(dsg_queue* q, int64_t ticket, dsg_queue_job_info* info);
int dsg_queue_info(dsg_queue* q, int64_t* rounds_total, int* n_pending, int* n_running);
int dsg_queue_cancel(dsg_queue* q, int64_t ticket);
int dsg_queue_close(dsg_queue* q);
/* host only, no device: exactly the placement the session follows */
int dsg_queue_place(const int32_t* K, const int32_t* arrive_round, int n_jobs, int n_slots,
                    int32_t* slot, int32_t* first_round, int32_t* n_rounds);
/* Live jobs: windows appended while the clip runs.  dsg_queue_submit wants all K audio windows of a job; a speaker who is still talking -- a
 * live avatar, a TTS stream, a call -- has them one by one.  A live job is submitted with a CAPACITY and is fed window by window; the window
 * hand-off (seed poses, root shift, one-frame blend) stays on the device, and the rows come back per window through rows_ready as for every
 * job.  The promise: a live job comes out bit for bit as dsg_sample_clip produces its K windows alone -- B = 1, its (seed, stream_id), its
 * skip, the same draw_base, root_shift / keep_last_tail and named kernel set, K = the windows it was finally given -- provided no window
 * changes the style or the scale; it does not matter when the windows arrived, how many rounds the job sat out, or what ran beside it.  (Window
 * c draws draw_base + c * (1 + n_run) and writes rows from c * (T - S) - S whatever K is.)  With a per-window style or scale it equals the
 * K-call sequence of this header: dsg_set_window_cond[_cfg] with that window's style and scale, dsg_sample, and the stitching of sample.py.
 * Reference counterpart: none.
 * dsg_queue_submit_live: job->K is the capacity, the most windows the job may ever get, and job->out is [n_out(capacity), J]; job->audio holds
 * the first n_given windows, contiguous (n_given == 0: may be NULL).  style, seed0, seed_last, scale, (seed, stream_id) and skip_timesteps
 * mean what they mean at dsg_queue_submit, whose per-job checks and messages apply; n_given outside [0, K]: DSG_E_INVALID.  A live job takes
 * no dsg_clip_edit: a constraint and an init motion are [n_out(K), J] tensors whose meaning depends on the final length (the cut tail of the
 * last window), which a live job does not know yet.
 * dsg_queue_append: n >= 1 further windows for a live job that is pending or running.  OWNERSHIP is the session's rule, per window: host
 * tensors (audio, style) are copied into session staging before the call returns; device tensors are read where they are, behind `stream`,
 * and must stay valid until windows_done has passed that window.  style NULL: the style of the window before it (window 0: the job's); scale
 * is read only with DSG_WIN_SCALE in a guided session and holds from that window on.  DSG_WIN_LAST on the last entry is dsg_queue_finish in
 * the same call.  DSG_E_INVALID, with the ticket in dsg_last_error: an unknown ticket, a job that is not live, a job that is finished, done
 * or cancelled, n < 1, a null audio, more windows than the capacity, DSG_WIN_LAST anywhere but on the last entry.  A refused call leaves
 * the job as it was.
 * dsg_queue_finish: the job's K becomes the number of windows given.  Windows still to run: the last of them runs as a clip's last window
 * and the job is DONE after that round.  Every given window has run already: the job is DONE before the call returns -- without
 * keep_last_tail rows_ready is K * (T - S) - S already; with it the closing S rows are copied from the slot's tail (the values the hand-off
 * kept for the next window's seed, after the shift) into rows [K * (T - S) - S, K * (T - S)), and on to a host `out`; the lane is drained.
 * No window ever given: the job is cancelled.  Finishing a finished job: no-op.  An unknown ticket or a job that is not live: DSG_E_INVALID.
 * PLACEMENT: a pending live job can be placed once it has a window; until then the tickets behind it pass it.  Once placed it keeps its slot
 * until it is finished or cancelled; first_round is the round of its window 0.  IDLE SLOT: a running live job without a window to run when
 * a round starts sits that round out -- dead for the round's start, draws, gather and hand-off; its y['seed'] rows, its tail and its state
 * stay; windows_done and rows_ready do not move.  dsg_queue_run returns early when no slot has a window to run and no pending job can be
 * placed: an idle live job alone runs no round.  rows_ready while live: min(n_out(capacity), windows_done * (T - S) - S); finished and done:
 * n_out(K); rows of `out` past n_out(K) are never written.  dsg_queue_job: windows_given / live (above).  Cancel, close and the ownership
 * of the lanes are unchanged.
 * On the device: k_window_handoff_q picks the two tail buffers per slot by the slot's window index (as dsg_sample_clip does), not by the
 * session's round, so a slot that sat out an odd number of rounds finds its tail where it left it; the gather table carries the style and
 * audio pointer of the window the slot stands on.
 * Added without a version step: dsg_version() stays 330; dsg_clip_job, dsg_clip_edit and dsg_queue_job_info keep their sizes. */
enum { DSG_WIN_SCALE = 1, DSG_WIN_LAST = 2 };
typedef struct dsg_queue_window {      /* 32 bytes */
    const float* audio;   /* [T_a, A_src]: ONE window, as dsg_set_window_cond takes it; required */
    const float* style;   /* [style_dim_in], or NULL: the style of the window before it (window 0: the job's) */
    float scale;          /* y['scale'] from this window on; read only with DSG_WIN_SCALE in a guided session */
    int32_t flags;        /* DSG_WIN_SCALE | DSG_WIN_LAST */
    int32_t reserved[2];
} dsg_queue_window;
int dsg_queue_submit_live(dsg_queue* q, const dsg_clip_job* job, int n_given, int skip_timesteps /* < 0: args->skip_timesteps */,
                          int64_t* ticket, void* stream);
int dsg_queue_append(dsg_queue* q, int64_t ticket, const dsg_queue_window* wins, int n, void* stream);
int dsg_queue_finish(dsg_queue* q, int64_t ticket);
/* Priorities, park and resume at window boundaries.  Placement above is first come, first served and a placed job keeps its slot until it
 * ends: a live speaker submitted while every slot holds a long batch clip waits for a clip to end, an idle live job keeps its slot as dead
 * rows, and a generation cannot be paused without cancelling it.  Between two rounds the only device state a running job owns is one [S][J]
 * fp32 block -- the tail its last window handed off -- and everything else a round needs (noise key and draw offsets, edits, skip,
 * conditioning, `out`) travels with the job.  So a job may leave its slot at a window boundary and continue later in any slot of any lane.
 * The promise stands: a job comes out bit for bit as dsg_sample_clip produces it alone -- B = 1, its (seed, stream_id), its skip and edits,
 * the same draw_base, root_shift / keep_last_tail and named kernel set -- however often it was parked and whichever slots and lanes it ran
 * in; for a live job with the provisos stated above.  Reference counterpart: none.
 * STATES: DSG_JOB_PARKED -- the job has run at least one window, holds no slot (slot == -1) and its hand-off state lives in session staging.
 * DSG_JOB_HELD (a bit of dsg_queue_job_info.live, for closed jobs too) -- the caller asked it to wait: a held PENDING job stays PENDING and
 * is not placed; a held RUNNING job is parked when dsg_queue_run next starts a round (or finds that none can start).  dsg_queue_job_info.
 * reserved[0] is `parks`, how often the job has been parked: 0 for every job never parked.  first_round stays the round of window 0;
 * windows_done, rows_ready and the rows already copied to a host `out` are untouched by parking.
 * dsg_queue_set_priority: default 0; higher runs first; read at the next placement.  dsg_queue_park: sets HELD.  dsg_queue_resume: clears it;
 * the job then competes for a slot like any waiting job.  All three: an unknown ticket -> DSG_E_INVALID with the ticket in dsg_last_error; a
 * DONE or CANCELLED job -> no-op, 0; park on a parked or held job, resume on a job that is not held -> no-op.  None of them touches the
 * device.
 * PLACEMENT, at the start of every round (this replaces the rule stated at dsg_queue_run; dsg_queue_place_prio is the same code on the host):
 *  1. the WAITING jobs are the PENDING and PARKED jobs that are not HELD and have a window to run (a live job without one cannot be placed),
 *     ordered by priority descending, then ticket ascending;
 *  2. the free slots, lowest first, take them in that order;
 *  3. then every waiting job W still unplaced, in order, looks among the running jobs NOT placed in this round for the victim V: the lowest
 *     priority; ties go first to a job without a window to run this round (an idle live job), then to the highest ticket.  If
 *     priority(V) < priority(W) strictly, V is parked and W takes its slot; otherwise the placement ends.
 * With all priorities equal and no HELD bit this is the rule above: the same slots, the same first_round, the same launches -- no copy and
 * no kernel is added to such a session -- and dsg_queue_place_prio(K, arrive, NULL, ...) gives dsg_queue_place's first_round.  There is
 * no ageing: a low priority starves for as long as higher ones keep the slots; that policy is the caller's.
 * dsg_queue_place_prio: host only.  K, arrive_round as dsg_queue_place; priority NULL: all 0.  first_round[j]: the round of window 0;
 * done_round[j]: the round of its last window; n_parks[j]: how often it is pre-empted; *n_rounds: one past the last done_round.  DSG_E_INVALID
 * as dsg_queue_place, and for a null output.
 * OTHER CALLS: dsg_queue_run returns early when nothing can run: held jobs alone, parked or pending, run no round.  dsg_queue_info:
 * n_pending counts PENDING + PARKED.  dsg_queue_cancel on a parked job releases its staging; dsg_queue_close abandons parked jobs as it does
 * running ones.  dsg_queue_finish on a parked live job whose given windows have all run: DONE before the call returns, as for a running
 * one; with keep_last_tail the closing S rows come from the parked block instead of the slot's tail.  A parked live job with windows left
 * waits for a slot like every parked job.
 * On the device.  Park: job V stands on window c in lane l, position p; clip_tail[(c - 1) & 1] + p * S * J of lane l is copied into a
 * staging block of the job (S * J * 4 bytes) on lane l's stream, in front of that lane's gather for the round -- whoever takes the slot
 * overwrites y['seed'] and the tail only behind it in stream order.  Resume into lane l', position p': k_clipq_gather, in the launch that
 * gathers the slot's style and audio, writes both images the hand-off would have left -- clip_tail[(c - 1) & 1][p'][s][j] and, transposed,
 * y['seed'][p'][j][s]; variant 5 gathers the job's y['seed_last'] again.  When l' != l, lane l''s stream waits on an event recorded behind
 * the park copy.  Slots that do not resume take the path they took before.
 * Added without a version step: dsg_version() stays 330; dsg_clip_job, dsg_clip_edit, dsg_queue_window and dsg_queue_job_info keep their
 * sizes and layouts. */
enum { DSG_JOB_PARKED = 4 };      /* dsg_queue_job_info.state */
enum { DSG_JOB_HELD = 4 };        /* bit of dsg_queue_job_info.live, beside DSG_JOB_LIVE | DSG_JOB_FINISHED */
int dsg_queue_set_priority(dsg_queue* q, int64_t ticket, int32_t priority);
int dsg_queue_park(dsg_queue* q, int64_t ticket);
int dsg_queue_resume(dsg_queue* q, int64_t ticket);
int dsg_queue_place_prio(const int32_t* K, const int32_t* arrive_round /* NULL: all 0 */, const int32_t* priority /* NULL: all 0 */,
                         int n_jobs, int n_slots, int32_t* first_round, int32_t* done_round, int32_t* n_parks, int32_t* n_rounds);
/* Per-element noise streams ("keyed noise") for dsg_sample / _multi / dsg_sample_clip / _multi.  seeds, stream_ids: HOST uint64[B], copied by
 * the call.  While set, element b of the batch draws from its own pair (seed_b, sid_b): draw d at frame f, feature j is
 *   philox4x32_10(ctr = ((f * Jq + j) >> 2, d, sid_b lo, sid_b hi), key = (seed_b lo, seed_b hi)) + Box-Muller,   Jq = J rounded up to 4,
 * that is the [1, J, 1, T] tensor of (seed_b, sid_b): the batch term of the counter is 0 and the key is per element.  An element's noise is
 * therefore exactly the noise it gets sampled alone (B = 1, args->seed = seed_b, args->stream_id = sid_b), whichever batch, slot, lane or rank
 * it rides in.  Draw indices stay per call: draw_base for x_T / the q_sample noise, draw_base + 1 + i for step i, window c of a clip call from
 * draw_base + c * (1 + n_run).
 * seeds == NULL: every element uses args->seed.  stream_ids == NULL with seeds: stream id 0 for every element.  stream_ids == NULL && seeds ==
 * NULL: off (B ignored).  B < 1 or B > max_batch: DSG_E_INVALID.  Sticky; a dsg_clone starts without; every lane has its own.  While set,
 * args->stream_id is ignored and a sampling call needs the same B (else DSG_E_INVALID with both numbers).  With guidance B is the user batch
 * and the unconditional twins follow their element.  const_noise: element 0's stream for everyone.  step_noise / init_noise replace the draws
 * exactly as they do without.  A chain run in pieces (first_step / max_steps) uses the same streams in every piece.  Without this call every
 * draw is what it always was.  Reference counterpart: none (th.randn consumes one global generator, gaussian_diffusion.py:704, :542).
 * Added without a version step, as dsg_set_inpainting and dsg_set_clip_init: dsg_version() stays 330. */
int dsg_set_noise_streams(dsg_handle* h, const uint64_t* seeds, const uint64_t* stream_ids, int B);
/* Kernel set of a handle (DSG_KSET_*; sticky; clones inherit the source's at dsg_clone).  dsg_recommend_kernel_set: the set
 * measured fastest for `lanes` lanes of batch B advanced together (lanes = 1: what DSG_KSET_AUTO picks) -- several lanes share
 * the CUs and prefer the throughput-shaped sets earlier; the caller applies it to each lane.  dsg_last_kernel_set: the set the
 * last dsg_forward / dsg_sample of the handle ran. */
int dsg_set_kernel_set(dsg_handle* h, int set);
int dsg_get_kernel_set(dsg_handle* h, int* set);      /* the set in force (DSG_KSET_*), incl. a DSG_KSET environment pin */
int dsg_recommend_kernel_set(dsg_handle* h, int B, int lanes, int* set);
int dsg_last_kernel_set(dsg_handle* h, int* set);
int dsg_sync(dsg_handle* h);
/* time of the step loop of the last dsg_sample (HIP events on the handle's stream; AQL path: first doorbell to the completion
 * signal of the last packet), and its step count */
int dsg_last_sample_ms(dsg_handle* h, float* ms, int* n_steps);
/* how the step loop of the last dsg_sample was submitted: 0 = HIP launches, 1 = hand-written AQL packets, 2 = hipGraph replay */
int dsg_last_sample_path(dsg_handle* h, int* path);
/* 1 when the AQL packets of that loop carried no acquire / release fences: the buffers the loop writes live in uncached device
 * memory (default for handles of max_batch <= 16; DSG_UC=0 selects cached buffers + agent-scope fences) and the one-time
 * hand-off self-check of the device passed */
int dsg_last_sample_fence_free(dsg_handle* h, int* fence_free);
/* ABI 320.  The loop buffers of fence-free handles are sub-allocated from per-device arenas of uncached memory that the library
 * keeps across handles (a range that changed its caching attribute between two lives proved incoherent on MI355X / ROCm 7.2, so a
 * destroyed handle's blocks go back to the arena, not to hipFree).  dsg_trim hands every arena of `device` (< 0: all devices)
 * without a live block back to the HIP allocator -- for a long-lived service between bursts of work -- and reports the bytes
 * released / still held (either pointer may be null).  DSG_UC_POOL_CAP_MB (default 16384) bounds the arenas of a device; a handle
 * created past the cap gets cached loop buffers + fenced packets (dsg_last_sample_fence_free reports 0).  No reference counterpart
 * (torch's caching allocator: torch.cuda.empty_cache()).
 * HAZARD (stated, not solved): a trimmed range returns to the HIP allocator, i.e. the very recycling the pool exists to avoid can happen to
 * whoever allocates next -- a later uncached arena is fill / read-back checked before its first use, a CACHED allocation (the caller's tensors,
 * this library's weights) that lands on the range is not.  Call it between bursts, when no handle of the device is live or about to be
 * created, and prefer leaving the pool alone.  The caller's current HIP device is left as it was. */
int dsg_trim(int device, long long* bytes_released, long long* bytes_held);
/* the framework's noise stream as a tensor: out [B, J, 1, T] (device) = draw `draw` of (seed, stream_id), i.e. exactly the
 * noise the fused sampler uses for that draw index (x_T is draw_base, step i is draw_base + 1 + i).  Stands in for
 * th.randn / th.randn_like of gaussian_diffusion.py:704, :542 in the generic loop. */
int dsg_noise(float* out, int B, int J, int T, uint64_t seed, uint64_t stream_id, uint32_t draw, void* stream);
/* dsg_noise with per-element streams: out [B, J, 1, T] (device, or host), element b = draw `draw` of (seeds[b], stream_ids[b]) by the definition
 * of dsg_set_noise_streams -- bit for bit dsg_noise(B = 1, seeds[b], stream_ids[b], draw), and what the fused loops of a handle with those
 * streams consume for that draw index.  seeds, stream_ids: HOST uint64[B]; a NULL array reads as zeros.  Reference counterpart: none (th.randn
 * consumes one global generator, gaussian_diffusion.py:704, :542). */
int dsg_noise_streams(float* out, int B, int J, int T, const uint64_t* seeds, const uint64_t* stream_ids, uint32_t draw, void* stream);

/* ZEGGS pose vectors -> BVH (pose2bvh of main/process/process_zeggs_bvh.py:219-275 and what it calls; host code, no GPU).
 * poses: host [frames, 1141], dtype 0 = float32, 1 = float64.  mean / std (float64[1141], both or neither): the sampler's
 * normalised output is de-normalised first, `poses * clip(std, 0.01) + mean` (sample.py:320-326); NULL: poses are taken as
 * they are.  smoothing != 0: Savitzky-Golay (15, 2) per feature (frames >= 15).  Output: `length` = frames, 3 * frames BVH
 * frames at 60 fps, 75 joints, text identical in layout to the reference writer's.
 * _channels: the numbers only -- offsets [75 * 3] (frame-0 positions, may be NULL) and motion [3 * frames, 228] in file order.
 * _batch: n_clips clips of `frames` frames, one file each, formatted on several host threads. */
int dsg_pose2bvh(const void* poses, int dtype, int frames, const double* mean, const double* std, int smoothing, const char* outpath);
int dsg_pose2bvh_channels(const void* poses, int dtype, int frames, const double* mean, const double* std, int smoothing,
                          double* offsets, double* motion);
int dsg_pose2bvh_batch(const void* poses, int dtype, int n_clips, int frames, const double* mean, const double* std, int smoothing,
                       const char* const* outpaths);

/* fused sampler arithmetic on caller tensors (flat fp32 arrays of B*per_batch elements, per-batch scalars on host) */
int dsg_q_sample(float* out, const float* x_start, const float* noise, const float* sqrt_ac, const float* sqrt_1mac,
                 int B, int64_t per_batch, void* stream);
int dsg_predict_xstart_from_eps(float* out, const float* x_t, const float* eps, const float* sqrt_recip,
                                const float* sqrt_recipm1, int B, int64_t per_batch, void* stream);
int dsg_posterior_step(float* out, const float* x_start, const float* x_t, const float* noise, const float* coef1,
                       const float* coef2, const float* sigma_nz, int B, int64_t per_batch, void* stream);
/* coef: host float[B*5] = {sqrt_recip, sqrt_recipm1, sqrt(abar_prev), sqrt(1-abar_prev-sigma^2), nonzero*sigma} */
int dsg_ddim_step(float* out, const float* x_start, const float* x_t, const float* noise, const float* coef, int B,
                  int64_t per_batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSG_H_ */
