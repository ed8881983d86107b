// dsg_hip.cpp -- host side of libdsg_hip.so (C ABI in include/dsg.h): weight ingestion / repacking, per-window
// conditioning, the per-step launch sequence, hipGraph capture of the step loop, and the sampler entry points.
// See dsg_kernels.h for the kernels and the reference file:line each one replaces.
#include "dsg_fused.h"
#include "dsg_batched.h"
#include "dsg_stream.h"
#include "../../include/dsg.h"
#include "dsg_aql.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

using namespace dsg;

// ---------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(DSG_E_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_) + " @" +        \
                                           std::to_string(__LINE__));                                    \
    } while (0)
#define CHK(expr)                  \
    do {                           \
        int r_ = (expr);           \
        if (r_ != 0) return r_;    \
    } while (0)

extern "C" const char* dsg_last_error(void) { return g_err.c_str(); }
void dsg_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }      // for the other translation units of the library (dsg_bvh.cpp)
extern "C" int dsg_version(void) { return DSG_VERSION; }

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int rup(int a, int b) { return cdiv(a, b) * b; }

static bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// ---------------------------------------------------------------------------------------------------------
// schedule tables (float64), GaussianDiffusion.__init__ (main/diffusion/gaussian_diffusion.py:161-198)
// ---------------------------------------------------------------------------------------------------------
struct Sched {
    int n = 0;
    std::vector<double> betas, ac, acp, sqrt_ac, sqrt_1mac, sqrt_recip, sqrt_recipm1, pvar, plogvar, coef1, coef2;
    std::vector<int> tmap;
};
static int build_sched(const double* betas, int n, Sched& s) {
    if (n <= 0) return fail(DSG_E_INVALID, "schedule: n <= 0");
    s.n = n;
    s.betas.assign(betas, betas + n);
    for (int i = 0; i < n; ++i)
        if (!(betas[i] > 0.0 && betas[i] <= 1.0)) return fail(DSG_E_INVALID, "schedule: betas must be in (0, 1]");
    auto rs = [&](std::vector<double>& v) { v.resize(n); };
    rs(s.ac); rs(s.acp); rs(s.sqrt_ac); rs(s.sqrt_1mac); rs(s.sqrt_recip); rs(s.sqrt_recipm1); rs(s.pvar);
    rs(s.plogvar); rs(s.coef1); rs(s.coef2);
    double c = 1.0;
    for (int i = 0; i < n; ++i) { c *= (1.0 - betas[i]); s.ac[i] = c; }
    for (int i = 0; i < n; ++i) s.acp[i] = i == 0 ? 1.0 : s.ac[i - 1];
    for (int i = 0; i < n; ++i) {
        s.sqrt_ac[i] = std::sqrt(s.ac[i]);
        s.sqrt_1mac[i] = std::sqrt(1.0 - s.ac[i]);
        s.sqrt_recip[i] = std::sqrt(1.0 / s.ac[i]);
        s.sqrt_recipm1[i] = std::sqrt(1.0 / s.ac[i] - 1);
        s.pvar[i] = betas[i] * (1.0 - s.acp[i]) / (1.0 - s.ac[i]);
        s.coef1[i] = betas[i] * std::sqrt(s.acp[i]) / (1.0 - s.ac[i]);
        s.coef2[i] = (1.0 - s.acp[i]) * std::sqrt(1.0 - betas[i]) / (1.0 - s.ac[i]);
    }
    for (int i = 0; i < n; ++i) s.plogvar[i] = std::log(n > 1 ? s.pvar[i == 0 ? 1 : i] : s.pvar[0]);
    return 0;
}
extern "C" int dsg_schedule_tables(const double* betas, int n, double* out) {
    Sched s;
    CHK(build_sched(betas, n, s));
    const std::vector<double>* t[11] = {&s.betas, &s.ac, &s.acp, &s.sqrt_ac, &s.sqrt_1mac, &s.sqrt_recip,
                                        &s.sqrt_recipm1, &s.pvar, &s.plogvar, &s.coef1, &s.coef2};
    for (int k = 0; k < 11; ++k) memcpy(out + (size_t)k * n, t[k]->data(), sizeof(double) * n);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------------------------------------
struct RawT { float* d = nullptr; std::vector<int64_t> shape; size_t n = 0; };
struct Layer {
    void *Wqkv = nullptr, *Wo = nullptr, *W1 = nullptr, *W2 = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr, *g1 = nullptr, *be1 = nullptr, *g2 = nullptr,
          *be2 = nullptr;
};

// Everything derived from the checkpoint alone (raw tensors, packed weights, tables): owned jointly by a handle and its
// clones (dsg_clone) -- several sampling lanes of one GPU read ONE copy of the weights, which therefore stays resident in the
// XCDs' L2 slices no matter how many clips are in flight.
struct SharedWeights {
    std::vector<void*> allocs;
    ~SharedWeights() { for (void* p : allocs) (void)hipFree(p); }
};

// The encoder core of a handle: (latent_dim, heads, padded tokens), the shape the fused attention / feed-forward kernels are instantiated per.  Each tuple is
// written HERE and nowhere else; OTHER = every remaining shape dsg_create accepts (the generic TILE / BLOCK / LATENCY kernels serve it).  Which fused forms
// exist per (core, precision, ff_size, pose width): the predicates above auto_kernel_set; which instantiation: the launchers' switches, closed by no_inst
enum class Core { OTHER, C128, C256, C384, C512 };
static Core classify_core(int D, int H, int Tp) {
    if (H != 4) return Core::OTHER;
    if (D == 128 && Tp == 32) return Core::C128;      // tiny (test dims)
    if (D == 256 && Tp == 96) return Core::C256;      // ZEGGS
    if (D == 384 && Tp == 160) return Core::C384;     // BEAT (DSG+)
    if (D == 512 && Tp == 160) return Core::C512;     // TWH (DSG+)
    return Core::OTHER;
}

// The per-element noise streams of one step loop, as the noise block takes them (GemmArgs::dyn has the layout): B keys {seed lo, seed hi, stream
// lo, stream hi} (seeds == false: the seed words come from args->seed; const_noise: element 0's key for everyone).  offs / starts / holds are a
// clip queue's: with per-clip skip_timesteps a slot that starts `hold` loop indices into the round draws its steps at offs = starts - hold and its
// start at starts.  Null in every other keyed call: zeros, written with every keyed upload, so nothing of a queue's round outlives it on the device
struct NoiseTable {      // (host storage of the builder's)
    int B = 0; bool seeds = false;      // B == 0: unkeyed
    const unsigned *keys = nullptr, *offs = nullptr, *starts = nullptr; const int* holds = nullptr;
};
// What the last sampling call on a handle did: what the dsg_last_* exports read, and nothing else.  While a call runs, its facts live in its
// own storage (SampleJob; the sums of a clip's windows, of a queue's rounds); commit_report writes them here once per lane where the call
// succeeds, so a call that is refused or fails, and a dsg_queue_run without a round, leave the previous report whole
struct LastRun {
    bool sampled = false; int steps = 0;      // a sampling call has completed; its steps (a clip: K * n_run, a queue: the summed round lengths)
    int path = 0; bool nofence = false;       // of its last window / round: 0 HIP launches, 1 AQL packets, 2 hipGraph replay; packets without fences
    double host_ms = -1.0;                    // >= 0: taken on the host (the AQL clock; a sum over windows / rounds); < 0: events ev_t0 .. ev_t1, resolved when asked
    int kset = -1;                            // the kernel set of the last step; dsg_forward commits this alone (no sampling call); < 0: no step has run
};
struct dsg_handle {
    dsg_config cfg;
    int prec = 0, es = 4, kbk = 16;      // element size / k-block of the precision policy
    int J, T, S, D, As, A, W, L, H, hd, ff, Hl, hdl, ntok, Tp, Jp, Jq, Bmax, Ta, n_te;
    int KSin = 4;                        // split-K of the pose-embedding GEMM: one split per 256 pose features
    Core core = Core::OTHER;             // classify_core(D, H, Tp), set once at dsg_create
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    std::vector<void*> allocs;                       // per-lane buffers (state, activations, conditioning)
    std::vector<void*> allocs_uc;                    // ... those in uncached memory: returned to the process-wide pool, never to hipFree
    std::shared_ptr<SharedWeights> shared;           // checkpoint-derived buffers (see SharedWeights)
    bool alloc_shared = false;                       // dalloc target: true while loading / finalizing weights
    bool is_clone = false;
    std::map<std::string, RawT> raw;
    bool finalized = false, cond_set = false;
    int condB = 0;
    // weights
    void* Wp_in = nullptr; void* Wp_out = nullptr; float* b_out = nullptr;
    std::vector<Layer> layers;
    float *TE = nullptr, *TE2 = nullptr, *rcos = nullptr, *rsin = nullptr, *cbase = nullptr, *zero_bias = nullptr;
    // window conditioning
    float *emb1 = nullptr, *Cf = nullptr, *enc = nullptr, *cvec = nullptr;
    float *c_style = nullptr, *c_seed = nullptr, *c_audio = nullptr, *c_seed_last = nullptr;
    int seed_last_B = 0;                 // batch of the last dsg_set_seed_last (variant 5)
    unsigned char* mask = nullptr; int mb = 1; int nomask = 0;
    // classifier-free guidance (dsg_set_window_cond_cfg): cfgB user batch elements + their unconditional twins = condB rows
    int cfgB = 0; float* cfg_scale = nullptr;
    // inpainting constraint (dsg_set_inpainting, the only writer of inpB): inpB user batch elements in the state's layout [inpB][T][Jp]; 0 = off.  Allocated on first use
    int inpB = 0; float* inp32 = nullptr; unsigned char *inp_mask = nullptr, *inp_stage = nullptr;
    // window hand-off of dsg_sample_clip (k_window_handoff): the previous window's last S frames [B][S][J], two copies used in turn (a hand-off reads
    // one and writes the other), and the stitched clip when the caller's `out` is host memory.  Allocated on first use
    float* clip_tail[2] = {nullptr, nullptr}; float* clip_out = nullptr; size_t clip_out_cap = 0;
    // clip-level inpainting constraint (dsg_set_clip_inpainting): the library's own copy in the stitched clip's coordinates [cinpB][cinp_frames][J];
    // cinpB == 0: off.  Allocated on first use, grown when needed (cinp_cap elements).  dsg_sample_clip cuts window c's constraint out of it into
    // inp32 / inp_mask (k_clip_inp_window)
    int cinpB = 0, cinp_frames = 0; float* cinp_motion = nullptr; unsigned char* cinp_mask = nullptr; size_t cinp_cap = 0;
    // clip-level init motion (dsg_set_clip_init): the library's own copy [cinitB][cinit_frames][J] in the stitched clip's coordinates; cinitB == 0:
    // off.  Allocated on first use, grown when needed (cinit_cap elements).  Only dsg_sample_clip reads it (k_clip_x_in)
    int cinitB = 0, cinit_frames = 0; float* cinit_motion = nullptr; size_t cinit_cap = 0;
    LastRun last;                        // the report of the last sampling call (commit_report)
    int kset_req = DSG_KSET_AUTO;        // dsg_set_kernel_set: the kernel set every step of this handle runs (AUTO: by batch, select_kernels)
    // state / activations
    float *xs32 = nullptr, *partial = nullptr, *X0 = nullptr, *pre1 = nullptr, *pre2 = nullptr, *Xn = nullptr,
          *X1 = nullptr, *fwd_out = nullptr, *io_tmp = nullptr, *io_tmp2 = nullptr, *ext_noise = nullptr;
    size_t ext_noise_cap = 0;
    void *xsA = nullptr, *X0a = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *attn = nullptr, *hidden = nullptr;
    float* ffn_part = nullptr; size_t ffn_slab = 0;      // [4][ffn_slab] partial linear2 results of k_ffn_part
    void* X1a = nullptr;                 // LayerNorm1 rows in the GEMM type, fragment-major (k_attn_op -> linear1)
    int* ctr = nullptr;                  // scratch counter for diagnostics
    StepCtl* ctl = nullptr;              // device-resident step control (dsg_kernels.h: StepCtl)
    int* t_arr = nullptr; unsigned* dyn = nullptr;
    // per-element noise streams (dsg_set_noise_streams): nkB user batch elements, 0 = off; nkeys = their keys {seed lo, seed hi, stream lo,
    // stream hi} (nk_seeds == false: the seed words come from args->seed, per call).  dyn_host: the staging copy of `dyn` every sampling call uploads
    int nkB = 0; bool nk_seeds = false; std::vector<unsigned> nkeys, dyn_host;
    // What a lane holds for the rounds of a clip queue (dsg_sample_clip_queue*, dsg_queue_*; QueueRound fills all of it).  The device buffers
    // are allocated on first use (queue_lane_ready); the *_host vectors are the copies uploaded per round, which outlive the uploads
    struct Queue {
        float *style = nullptr, *audio = nullptr;      // the round's per-slot style / audio [Bmax][...]: what set_window_cond reads
        std::vector<float> scale_host;                 // ... and its per-slot guidance scale
        HandoffSlot* slots = nullptr; std::vector<HandoffSlot> slots_host;      // the hand-off table (k_window_handoff_q)
        EditSlot* edits = nullptr; std::vector<EditSlot> edits_host;            // the edit table (k_clipq_inp_window / k_clipq_x_in)
        GatherSlot* gather = nullptr; std::vector<GatherSlot> gather_host;      // the gather table of a session (k_clipq_gather)
        unsigned char* stage = nullptr; size_t stage_cap = 0;      // a one-shot call's host-side edit tensors, staged (grown when needed)
    } cq;
    // the queue session that owns this lane (dsg_queue_open .. dsg_queue_close): while set, owned_by_queue refuses every other sampling call
    struct dsg_queue* owner = nullptr;
    int latency_mode = -1;               // dsg_config.latency_mode: -1 auto, 0 never the LATENCY set, 1 always
#ifndef DSG_EMU
    dsg_aql::Ctx aql;                    // hand-written AQL submission of the step loop (dsg_aql.h)
#endif
    // Fence-free step loop (DSG_UC, default 1): every buffer the loop WRITES (state, activations, step control) lives in
    // uncached device memory (MTYPE UC: neither the CUs' L1 nor the XCDs' L2 hold its lines, so a kernel on any XCD reads what
    // the previous kernel wrote without cache maintenance), the step control is read with vector loads (never through the
    // scalar cache), and the AQL packets of the loop carry NO acquire / release fence (first packet acquires, last releases).
    // Weights, tables and conditioning stay in cached memory -- nothing writes them during the loop.  Measured on MI355X
    // (profiles/r02_q_*): the fences are worth ~6 us per batch-1 step, the uncached buffers cost ~3 (117 us with uncached buffers
    // behind the usual fences, DSG_UC=2): 111.0 vs 114.2 us/step, bit-identical samples; 16 clips in 4 lanes: 5628 vs 5120 frames/s.
    // DSG_UC=0: cached buffers, agent-scope fences.  HIP launches / hipGraph keep the runtime's own fences either way.
    // The first fence-free run of a process checks the premise on the device it runs on (uc_selfcheck) and falls back to fenced
    // packets with a warning if a hand-off through uncached memory is ever seen stale.
    int uc_mode = 1;
    bool alloc_uc = false;               // dalloc target: a loop-written buffer
    bool state_fences = false;           // the state lives in cached memory: release on the step's last packet, acquire on its first
    int fence_next = 0;                  // step_launch: the next recorded packet acquires (1) / releases (2) at agent scope
    int aql_mode = 1;                    // DSG_AQL: 1 (default) = AQL packets for the eager step loop, 0 = HIP launches
    bool aql_warned = false;
    // A/B switches of the batched sets, read ONCE at dsg_create (round-4 advisor: they used to be getenv calls in select_kernels /
    // run_step, i.e. in the hot path and outside the hipGraph key): -1 = not set
    int env_loc64_from = 2048;           // DSG_LOC64_FROM=<workgroups>: k_loc as two waves per (head, window, clip) from that many of them (test hook / A/B)
    int env_ffn_rt4 = -1;                // DSG_FFN_RT4=<rows>: k_ffn on 64-row blocks from that many token rows at any lane count (0: never)
    int env_ffn_split = -1;              // DSG_FFN_SPLIT=0: linear1 + linear2 + LayerNorm-on-read instead of k_ffn_part + k_ffn_ln (BLOCK)
    int env_clip_attn = -1;              // DSG_CLIP_ATTN=0: QKV GEMM + k_attn_op instead of k_clip_attn + k_ffn_ln (BLOCK; differs in the last bits)
    int* st_tmodel = nullptr; float* st_c[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int st_cap = 0, n_run = 1;
    bool st_valid = false; int st_mode = -1, st_skip = -1; float st_eta = 0.f;      // what the device tables hold
    Sched sched;
    // graphs: key = (B, out_mode, mask batch, const_noise, steps, flags, kernel set) -> exec
    // (flags: 1 clip_denoised, 2 guidance, 4 no mask_local, 8 k_attn_mid, 16 no noise, 32 inpainting on -- the captured pose head carries the constraint's pointers, 64 keyed noise)
    // n_run is part of the key: the captured kernels carry the step-table length as an argument (n_tab); so is the kernel set
    // (a graph captured under one set must never be replayed for a call that asked for another)
    // (round-4 advisor: n_run = the steps of THIS call, n_tab = the length of the whole chain = what the captured kernels clamp their
    // step-table reads with -- a chain run in pieces, first_step / max_steps, has n_run < n_tab, so both are part of the key)
    struct GKey { int B, mode, mb, cn, n_run, n_tab, flags, kset; bool operator<(const GKey& o) const {
        return std::tie(B, mode, mb, cn, n_run, n_tab, flags, kset) < std::tie(o.B, o.mode, o.mb, o.cn, o.n_run, o.n_tab, o.flags, o.kset); } };
    struct GVal { hipGraphExec_t exec; hipGraph_t graph; int steps; };
    std::map<GKey, GVal> graphs;
};

// bf16 activations (DSG_PREC_BF16, DSG_PREC_BF16W2): the compute-dtype shadows / fragment layouts of the bf16 kernels
// a lane of an open queue session belongs to it: DSG_E_STATE for whoever else wants to sample on it or change its state
static int owned_by_queue(const dsg_handle* h) { return h && h->owner ? fail(DSG_E_STATE, "handle belongs to an open queue") : 0; }
static inline bool is_bf16(const dsg_handle* h) { return h->prec != DSG_PREC_FP32; }
static inline bool core_narrow(const dsg_handle* h) { return h->core == Core::C128 || h->core == Core::C256; }      // the ZEGGS / tiny widths
static inline bool core_wide(const dsg_handle* h) { return h->core == Core::C384 || h->core == Core::C512; }        // the DSG+ widths
// the closed end of every launcher that switches on the core: select_kernels / check_set let no such call through
static int no_inst(const dsg_handle* h, const char* kernel) {
    return fail(DSG_E_NOT_IMPLEMENTED, std::string(kernel) + ": no instantiation for (latent_dim, heads, padded tokens) = (" + std::to_string(h->D) + ", " +
                                           std::to_string(h->H) + ", " + std::to_string(h->Tp) + ") in precision " + std::to_string(h->prec));
}

// Uncached device memory is never handed back to the HIP allocator while a handle may still be created (round 4).  Found with
// tools/debug_rowdep*.py: after a handle with uncached loop buffers had been destroyed, a NEW handle whose buffers landed on the
// recycled range computed wrong rows (tiny dims, batch 200 after a batch-170 handle: every frame row >= 4096 -- exactly the part of
// `partial` beyond its first 2 MiB -- off by up to 100 %; DSG_UC=0 clean; same under every kernel set) -- memory that changed its
// caching attribute between two lives is not reliably coherent.
// Round 5 (verdict 8c / advisor): the pool is a SUB-ALLOCATOR over large arenas that stay uncached for their whole life (first fit,
// free neighbours coalesced), so a long-lived process that creates and destroys handles of varying max_batch holds the peak of what
// was alive at once, not the sum of every size class it ever asked for; DSG_UC_POOL_CAP_MB (default 16384) bounds the arenas of a
// device -- past it a handle gets cached loop buffers + fenced packets; dsg_trim() hands arenas without a live block back to HIP.
// Every FRESH arena is filled and read back by two kernels before its first use (uc_arena_ok): that is the observed symptom of a
// recycled range (wrong values between dependent launches), tested where it would show; a failing arena is quarantined (kept, never
// used, never freed) and another one is tried.
struct UcArena {
    char* base = nullptr; size_t size = 0, used = 0;
    std::map<size_t, size_t> free;       // offset -> length of the free runs
    bool quarantined = false;
};
struct UcPool {
    std::mutex mu;
    std::vector<UcArena> arenas[64];     // per device
    std::map<void*, std::pair<char*, size_t>> live;    // block -> (base of its arena, length)
    size_t trimmed = 0;                  // arenas returned by dsg_trim so far (diagnostics)
    // (allocation time only -- handle creation, never the step loop -- so the cap is read where it is applied)
    static size_t cap_bytes() { const char* e = getenv("DSG_UC_POOL_CAP_MB"); return (size_t)(e ? std::max(atoll(e), 0ll) : 16384ll) << 20; }
};
static UcPool& uc_pool() { static UcPool* p = new UcPool(); return *p; }      // (leaked on purpose: arenas outlive every handle)
constexpr size_t UC_ALIGN = 4096, UC_ARENA_MIN = (size_t)32 << 20, UC_ARENA_GRAN = (size_t)2 << 20;
#ifndef DSG_EMU
__global__ void k_uc_fill(unsigned* p, size_t n, unsigned salt) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (unsigned)i * 2654435761u + salt;
}
__global__ void k_uc_verify(const unsigned* p, size_t n, unsigned salt, unsigned* bad) {
    unsigned b = 0;
    // (read by OTHER workgroups than the ones that wrote: the grid is walked from the far end)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t j = n - 1 - i;
        b += p[j] != (unsigned)j * 2654435761u + salt;
    }
    if (b) atomicAdd(bad, b);
}
// fill + read-back of a whole fresh arena, twice with different patterns, through ordinary launches on the null stream
static bool uc_arena_ok(char* base, size_t size) {
    unsigned* bad = nullptr;
    if (hipMalloc((void**)&bad, sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); return false; }
    bool ok = hipMemset(bad, 0, sizeof(unsigned)) == hipSuccess;
    const size_t n = size / sizeof(unsigned);
    for (unsigned pass = 0; pass < 2 && ok; ++pass) {
        hipLaunchKernelGGL(k_uc_fill, dim3(1024), dim3(256), 0, 0, (unsigned*)base, n, 0x9E3779B9u * (pass + 1));
        hipLaunchKernelGGL(k_uc_verify, dim3(1024), dim3(256), 0, 0, (const unsigned*)base, n, 0x9E3779B9u * (pass + 1), bad);
        ok = hipGetLastError() == hipSuccess;
    }
    unsigned nbad = 1;
    ok = ok && hipMemcpy(&nbad, bad, sizeof nbad, hipMemcpyDeviceToHost) == hipSuccess && nbad == 0;
    (void)hipFree(bad);
    return ok;
}
#endif
// a block of `bytes` of uncached memory on device `dev`, or nullptr (no uncached memory here / pool cap reached)
static void* uc_pool_take(int dev, size_t bytes, bool ignore_cap = false) {
#ifdef DSG_EMU
    (void)dev; (void)bytes; (void)ignore_cap;
    return nullptr;
#else
    UcPool& P = uc_pool();
    std::lock_guard<std::mutex> lock(P.mu);
    auto& av = P.arenas[dev & 63];
    bytes = (bytes + UC_ALIGN - 1) / UC_ALIGN * UC_ALIGN;
    for (int attempt = 0; attempt < 4; ++attempt) {
        for (size_t ai = 0; ai < av.size(); ++ai) {
            UcArena& A = av[ai];
            if (A.quarantined) continue;
            for (auto it = A.free.begin(); it != A.free.end(); ++it)
                if (it->second >= bytes) {
                    const size_t off = it->first, len = it->second;
                    A.free.erase(it);
                    if (len > bytes) A.free.emplace(off + bytes, len - bytes);
                    A.used += bytes;
                    P.live[A.base + off] = {A.base, bytes};
                    return A.base + off;
                }
        }
        size_t total = 0;
        for (const UcArena& A : av) total += A.size;
        const size_t want = std::max(UC_ARENA_MIN, (bytes + UC_ARENA_GRAN - 1) / UC_ARENA_GRAN * UC_ARENA_GRAN);
        if (!ignore_cap && total + want > UcPool::cap_bytes()) return nullptr;
        void* d = nullptr;
        // (round 6, measured no: FINE-GRAINED device memory instead of uncached is cached non-coherently across the XCDs -- the hand-off self-check
        //  fails with 4 M stale words, the fences come back: 16 clips 204 -> 221 us per step, profiles/r06_e_finegrained_vs_uncached.log)
        if (hipExtMallocWithFlags(&d, want, hipDeviceMallocUncached) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        UcArena A;
        A.base = (char*)d; A.size = want;
        A.quarantined = !uc_arena_ok(A.base, want);
        if (A.quarantined)
            fprintf(stderr, "libdsg_hip: WARNING: a fresh %zu MB range of uncached device memory failed its fill / read-back check on device %d; "
                            "quarantined (kept, never used)\n", want >> 20, dev);
        else A.free.emplace(0, want);
        av.push_back(std::move(A));
    }
    return nullptr;
#endif
}
static void uc_pool_give(int dev, void* d) {
    UcPool& P = uc_pool();
    std::lock_guard<std::mutex> lock(P.mu);
    auto lv = P.live.find(d);
    if (lv == P.live.end()) return;
    UcArena* Ap = nullptr;
    for (UcArena& X : P.arenas[dev & 63]) if (X.base == lv->second.first) Ap = &X;
    if (!Ap) return;
    UcArena& A = *Ap;
    size_t off = (size_t)((char*)d - A.base), len = lv->second.second;
    P.live.erase(lv);
    A.used -= len;
    auto nx = A.free.lower_bound(off);
    if (nx != A.free.end() && off + len == nx->first) { len += nx->second; nx = A.free.erase(nx); }
    if (nx != A.free.begin()) {
        auto pv = std::prev(nx);
        if (pv->first + pv->second == off) { off = pv->first; len += pv->second; A.free.erase(pv); }
    }
    A.free.emplace(off, len);
}
// Hands every arena of `device` that holds no live block back to the HIP allocator (device < 0: all devices) and reports the bytes
// still held.  Meant for a long-lived service between bursts of work; arenas allocated afterwards are checked like any fresh one.
extern "C" int dsg_trim(int device, long long* bytes_released, long long* bytes_held) {
    UcPool& P = uc_pool();
    int dev_before = -1;
    if (hipGetDevice(&dev_before) != hipSuccess) { (void)hipGetLastError(); dev_before = -1; }
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{dev_before};      // the caller's current device is left as it was
    std::lock_guard<std::mutex> lock(P.mu);
    long long rel = 0, held = 0;
    for (int dev = 0; dev < 64; ++dev) {
        if (device >= 0 && dev != (device & 63)) { for (const UcArena& A : P.arenas[dev]) held += (long long)A.size; continue; }
        auto& av = P.arenas[dev];
        bool any = false;
        for (const UcArena& A : av) any = any || (A.used == 0 && !A.quarantined);
        if (!any) { for (const UcArena& A : av) held += (long long)A.size; continue; }
        HIPCHK(hipSetDevice(dev));
        HIPCHK(hipDeviceSynchronize());
        std::vector<UcArena> keep;
        for (size_t ai = 0; ai < av.size(); ++ai) {
            if (av[ai].used == 0 && !av[ai].quarantined) { (void)hipFree(av[ai].base); rel += (long long)av[ai].size; ++P.trimmed; }
            else { held += (long long)av[ai].size; keep.push_back(std::move(av[ai])); }
        }
        av = std::move(keep);
    }
    if (bytes_released) *bytes_released = rel;
    if (bytes_held) *bytes_held = held;
    return 0;
}
template <class T>
static int dalloc(dsg_handle* h, T** p, size_t n_elems, bool zero = true) {
    void* d = nullptr;
    size_t bytes = n_elems * sizeof(T);
    if (bytes == 0) bytes = 16;
    bool is_uc = false;
#ifndef DSG_EMU
    if (h->uc_mode && h->alloc_uc && !h->alloc_shared) {
        d = uc_pool_take(h->cfg.device, bytes);
        if (!d) h->uc_mode = 0;          // no uncached memory here (or the pool's cap is reached): cached buffers, fenced packets
        is_uc = d != nullptr;
    }
#endif
    if (!d) HIPCHK(hipMalloc(&d, bytes));
    // Zero-fill and WAIT for it.  hipMemset on device memory may return before the fill has run; the handle's stream is
    // non-blocking (no implicit ordering with the null stream), so a late fill could wipe what the first kernels on the
    // handle's stream (weight packing, conditioning) or a following synchronous copy have already written.  Seen once
    // as a wrong TWH forward in a full `pytest -m gpu` run.  Allocation happens at create / load time only.
    if (zero) {
        HIPCHK(hipMemsetAsync(d, 0, bytes, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (h->alloc_shared) h->shared->allocs.push_back(d);
    else if (is_uc) h->allocs_uc.push_back(d);
    else h->allocs.push_back(d);
    *p = (T*)d;
    return 0;
}
// A per-lane block that grows with its use (the clip-level copies, the queue's staging): the old one goes back at once -- the stream is
// drained, nothing on it may still read it -- and *p becomes n_elems long, not zeroed.  The caller keeps the capacity
template <class T>
static int regrow(dsg_handle* h, T** p, size_t n_elems) {
    HIPCHK(hipStreamSynchronize(h->stream));
    if (void* old = *p) {
        *p = nullptr;
        h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), old), h->allocs.end());
        (void)hipFree(old);
    }
    return dalloc(h, p, n_elems, false);
}
static int dalloc_bytes(dsg_handle* h, void** p, size_t bytes) {
    unsigned char* d = nullptr;
    CHK(dalloc(h, &d, bytes));
    *p = d;
    return 0;
}

// expected checkpoint tensors (name -> shape); the reference's state_dict contract
static std::map<std::string, std::vector<int64_t>> expected_tensors(const dsg_handle* h) {
    std::map<std::string, std::vector<int64_t>> m;
    const int64_t D = h->D, J = h->J, S = h->S, A = h->A, As = h->As, ff = h->ff;
    m["WavEncoder.audio_feature_map.weight"] = {A, As};
    m["WavEncoder.audio_feature_map.bias"] = {A};
    m["sequence_pos_encoder.pe"] = {h->cfg.pe_max_len, 1, D};
    m["input_process.poseEmbedding.weight"] = {D, J};
    m["input_process.poseEmbedding.bias"] = {D};
    for (int i = 0; i < h->L; ++i) {
        const std::string p = "seqTransEncoder.layers." + std::to_string(i) + ".";
        m[p + "self_attn.in_proj_weight"] = {3 * D, D};
        m[p + "self_attn.in_proj_bias"] = {3 * D};
        m[p + "self_attn.out_proj.weight"] = {D, D};
        m[p + "self_attn.out_proj.bias"] = {D};
        m[p + "linear1.weight"] = {ff, D};
        m[p + "linear1.bias"] = {ff};
        m[p + "linear2.weight"] = {D, ff};
        m[p + "linear2.bias"] = {D};
        m[p + "norm1.weight"] = {D}; m[p + "norm1.bias"] = {D};
        m[p + "norm2.weight"] = {D}; m[p + "norm2.bias"] = {D};
    }
    m["embed_timestep.time_embed.0.weight"] = {D, D};
    m["embed_timestep.time_embed.0.bias"] = {D};
    m["embed_timestep.time_embed.2.weight"] = {D, D};
    m["embed_timestep.time_embed.2.bias"] = {D};
    if (h->cfg.variant == 3) {
        m["embed_style.weight"] = {64, h->cfg.style_dim_in};
        m["embed_style.bias"] = {64};
        m["embed_text.weight"] = {D - 64, J * S};
        m["embed_text.bias"] = {D - 64};
    } else {
        m["embed_style.weight"] = {D, h->cfg.style_dim_in};
        m["embed_style.bias"] = {D};
        m["embed_text.weight"] = {A, J};
        m["embed_text.bias"] = {A};
        if (h->cfg.variant == 5) {          // DiffuseStyleGesture++ (BEAT-TWH mdm.py:85-89)
            m["embed_text_last.weight"] = {A, J};
            m["embed_text_last.bias"] = {A};
        }
    }
    m["output_process.poseFinal.weight"] = {J, D};
    m["output_process.poseFinal.bias"] = {J};
    m["rel_pos.inv_freq"] = {h->hdl / 2};
    m["input_process2.weight"] = {D, 2 * D + A};
    m["input_process2.bias"] = {D};
    return m;
}

static bool stream_set_ok(const dsg_handle* h);
static bool rows_w2_ok(const dsg_handle* h);
extern "C" int dsg_create(const dsg_config* c, dsg_handle** out) {
    if (!c || !out) return fail(DSG_E_INVALID, "dsg_create: null argument");
    if (c->variant < 3 || c->variant > 5) return fail(DSG_E_NOT_IMPLEMENTED, "variant must be 3, 4 or 5");
    if (c->variant == 5 && c->n_poses <= 2 * c->n_seed) return fail(DSG_E_INVALID, "variant 5 needs n_poses > 2 * n_seed");
    if (c->latent_dim % 64 || c->latent_dim > 512 || c->latent_dim <= 0)
        return fail(DSG_E_INVALID, "latent_dim must be a multiple of 64, <= 512");
    if (c->variant == 3 && c->latent_dim <= 64) return fail(DSG_E_INVALID, "variant 3 needs latent_dim > 64");
    if (c->window <= 0 || c->window > 16 || c->n_poses % c->window)
        return fail(DSG_E_INVALID, "n_poses must be a multiple of window (<= 16)");
    if (c->num_heads <= 0 || c->latent_dim % c->num_heads) return fail(DSG_E_INVALID, "num_heads");
    const int hd = c->latent_dim / c->num_heads;
    if (!(hd == 32 || hd == 64 || hd == 96 || hd == 128)) return fail(DSG_E_INVALID, "self-attention head dim must be 32/64/96/128");
    if (c->local_heads <= 0 || c->latent_dim % c->local_heads) return fail(DSG_E_INVALID, "local_heads");
    const int hdl = c->latent_dim / c->local_heads;
    if (hdl > 64 || (hdl & 1)) return fail(DSG_E_INVALID, "local head dim must be even and <= 64");
    if (c->ff_size % 128 || c->ff_size <= 0) return fail(DSG_E_INVALID, "ff_size must be a multiple of 128");
    if (c->audio_dim % 4) return fail(DSG_E_INVALID, "audio_dim must be a multiple of 4");
    if (c->max_batch <= 0 || c->njoints <= 0 || c->n_seed < 0 || c->n_seed >= c->n_poses)
        return fail(DSG_E_INVALID, "bad dims");
    if (c->precision != DSG_PREC_FP32 && c->precision != DSG_PREC_BF16 && c->precision != DSG_PREC_BF16W2) return fail(DSG_E_INVALID, "precision");
#ifdef DSG_DEV_BF16_ONLY
    if (c->precision != DSG_PREC_BF16) return fail(DSG_E_NOT_IMPLEMENTED, "development build (make dev): bf16 only");
#endif
    const int ntok = c->n_poses + 1, Tp = rup(ntok, 32);
    if (!(Tp == 32 || Tp == 96 || Tp == 160))
        return fail(DSG_E_NOT_IMPLEMENTED, "attention kernel is instantiated for n_poses+1 padded to 32, 96 or 160 tokens");
    // (the kernels index rows and features in 32 bits on the 24-bit multiplier -- dsg_kernels.h: imul24)
    {
        const size_t widest = (size_t)std::max(std::max(c->ff_size, c->latent_dim), (c->njoints + 127) / 128 * 128);
        if ((size_t)c->max_batch * (size_t)ntok >= ((size_t)1 << 23) || (size_t)c->max_batch * (size_t)ntok * widest >= ((size_t)1 << 30))
            return fail(DSG_E_INVALID, "max_batch too large: token rows x widest row must stay below 2^30 elements (use several lanes / handles)");
    }
    HIPCHK(hipSetDevice(c->device));

    dsg_handle* h = new dsg_handle();
    h->shared = std::make_shared<SharedWeights>();
    h->cfg = *c;
    h->prec = c->precision;
    h->es = is_bf16(h) ? 2 : 4;
    h->kbk = is_bf16(h) ? 32 : 16;
    h->J = c->njoints; h->T = c->n_poses; h->S = c->n_seed; h->D = c->latent_dim; h->As = c->audio_src_dim;
    h->A = c->audio_dim; h->W = c->window; h->L = c->num_layers; h->H = c->num_heads; h->hd = hd; h->ff = c->ff_size;
    h->Hl = c->local_heads; h->hdl = hdl; h->ntok = ntok; h->Tp = Tp;
    h->Jp = rup(h->J, 128); h->Jq = rup(h->J, 4); h->Bmax = c->max_batch;
    h->KSin = cdiv(h->Jp, 256);
    h->core = classify_core(h->D, h->H, h->Tp);
    h->Ta = c->variant == 3 ? h->T : h->T - h->S * (c->variant == 5 ? 2 : 1);
    h->n_te = c->train_steps > 0 ? c->train_steps : 1000;
    if (h->n_te > c->pe_max_len) { delete h; return fail(DSG_E_INVALID, "train_steps > pe_max_len"); }
    h->layers.resize(h->L);
    h->latency_mode = c->latency_mode == 1 ? 0 : (c->latency_mode == 2 ? 1 : -1);
    // Environment switches of the release library (everything else is an API / config field):
    //   DSG_KSET  kernel set for every handle (1 latency, 2 tile, 3 block, 4 stream; overrides dsg_set_kernel_set)   [A/B runs]
    //   DSG_UC    0: cached loop buffers + fenced packets, 1: uncached + fence-free, 2: uncached + fenced
    //   DSG_AQL   0: HIP launches instead of hand-written AQL packets
    if (const char* e = getenv("DSG_KSET")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end != 0 || v < DSG_KSET_AUTO || v > DSG_KSET_ROWS) {
            delete h;
            return fail(DSG_E_INVALID, std::string("DSG_KSET must be 0 (auto) .. 5 (rows), got '") + e + "'");
        }
        h->kset_req = (int)v;
    }
    // Large batches on the BLOCK set re-read their activations from the L2 often enough that the uncached buffers cost what the
    // fences save (4 x 16: 9667 vs 9680 frames/s, 4 x 32: 10 430 vs 10 695): cached + fenced from batch 17 -- unless the handle can run
    // the STREAM set, which large batches select and which reads an activation block once per 128-column panel: fence-free wins there
    // at every size (1 x 64: 505 -> 479 us, 1 x 32: 356 -> 338, 4 x 32: 13.3k -> 13.8k frames/s; profiles/r03_q_uc_stream.log)
    if (c->max_batch > 16 && !stream_set_ok(h) && !rows_w2_ok(h)) h->uc_mode = 0;      // (bf16w2: ROWS at these sizes, every activation read once per workgroup)
    if (const char* e = getenv("DSG_UC")) h->uc_mode = atoi(e);
    if (const char* e = getenv("DSG_AQL")) h->aql_mode = atoi(e);
    else {
        // under a profiler the HSA queues are intercepted and rewritten (rocprofv3 crashed on hand-written packets), so
        // profiled runs use the HIP launches -- the same kernels, visible to the tool
        for (const char* v : {"ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB", "ROCPROFILER_REGISTER_FORCE_LOAD", "ROCPROF_COUNTER_COLLECTION", "ROCPROF_KERNEL_TRACE", "LD_PRELOAD"}) {
            const char* val = getenv(v);
            if (val && (strstr(val, "rocprof") || strstr(v, "ROCPROF"))) h->aql_mode = 0;
        }
    }
    if (const char* e = getenv("DSG_FFN_RT4")) h->env_ffn_rt4 = std::max(atoi(e), 0);
    if (const char* e = getenv("DSG_LOC64_FROM")) h->env_loc64_from = std::max(atoi(e), 1);
    if (const char* e = getenv("DSG_FFN_SPLIT")) h->env_ffn_split = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("DSG_CLIP_ATTN")) h->env_clip_attn = atoi(e) != 0 ? 1 : 0;
    *out = h;

    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&h->ev_t0));
    HIPCHK(hipEventCreate(&h->ev_t1));

    const int B = h->Bmax, D = h->D;
    // row buffers carry one extra padded token block: the fused attention kernel reads Tp rows per batch element
    // (+64: the block GEMMs of dsg_batched.h read and LayerNorm whole 64-row blocks)
    const size_t Min_pad = rup(B * h->T, 16) + 16 + 128, M_pad = rup(B * ntok, 16) + Tp + 128;
    // The sampler STATE (x_t fp32 + its bf16 shadow) is the one loop-written buffer that crosses a STEP boundary only: written by
    // the last kernel of a step, read by the first (and last) kernel of the next.  It stays in cached memory and exactly those two
    // packets carry an agent-scope release / acquire (state_fences): the timeline of the fence-free path
    // (profiles/r03_aql_step_timeline_b16.json) showed 11.6 us between the pose head's last wave and the next step's first wave at
    // batch 16 -- 9.8 MB of state written as uncached stores have to be acknowledged one by one -- against ~1 us for a plain
    // boundary; a write-back of the same bytes from the L2 costs 1-2 us.  DSG_STATE_UC=1: the round-2 behaviour (state uncached).
    h->state_fences = h->uc_mode == 1 && !(getenv("DSG_STATE_UC") && atoi(getenv("DSG_STATE_UC")));
    h->alloc_uc = !h->state_fences;
    CHK(dalloc(h, &h->xs32, (size_t)B * h->T * h->Jp + 16 * h->Jp));
    if (is_bf16(h)) CHK(dalloc_bytes(h, &h->xsA, ((size_t)Min_pad * h->Jp) * h->es));
    h->alloc_uc = true;                  // ---- written AND read inside one step by the kernels of the loop
    CHK(dalloc(h, &h->partial, (size_t)h->KSin * Min_pad * D));
    CHK(dalloc(h, &h->X0, M_pad * D));
    CHK(dalloc_bytes(h, &h->X0a, M_pad * D * h->es * (h->prec == DSG_PREC_BF16W2 ? 2 : 1)));      // (bf16w2, ROWS: hi + lo images)
    CHK(dalloc(h, &h->pre1, M_pad * D));
    CHK(dalloc(h, &h->pre2, M_pad * D));
    CHK(dalloc(h, &h->Xn, M_pad * D));
    CHK(dalloc(h, &h->X1, M_pad * D));
    CHK(dalloc_bytes(h, &h->attn, M_pad * D * h->es * (h->prec == DSG_PREC_BF16W2 ? 2 : 1)));      // (bf16w2: hi + lo images)
    CHK(dalloc_bytes(h, &h->X1a, M_pad * D * h->es));
    CHK(dalloc_bytes(h, &h->hidden, M_pad * (size_t)h->ff * h->es * (h->prec == DSG_PREC_BF16W2 ? 2 : 1)));      // (bf16w2: hi + lo images)
    h->ffn_slab = M_pad * D;             // (the partial linear2 slabs of k_ffn_part are allocated on the first BLOCK call: ensure_set_buffers)
    const size_t qkv_elems = (size_t)B * h->H * Tp * hd;
    CHK(dalloc_bytes(h, &h->q, qkv_elems * h->es));
    CHK(dalloc_bytes(h, &h->k, qkv_elems * h->es));
    CHK(dalloc_bytes(h, &h->vt, qkv_elems * h->es));
    CHK(dalloc(h, &h->ctl, 1));
    h->alloc_uc = false;                 // ---- inputs / outputs / conditioning: constant while the loop runs
    CHK(dalloc(h, &h->fwd_out, (size_t)B * h->J * h->T));
    CHK(dalloc(h, &h->io_tmp, (size_t)B * h->J * h->T));
    CHK(dalloc(h, &h->io_tmp2, (size_t)B * h->J * h->T));
    CHK(dalloc(h, &h->emb1, (size_t)B * D));
    CHK(dalloc(h, &h->cvec, (size_t)B * D));
    CHK(dalloc(h, &h->Cf, (size_t)B * h->T * D));
    CHK(dalloc(h, &h->enc, (size_t)B * h->T * h->A));
    CHK(dalloc(h, &h->c_style, (size_t)B * c->style_dim_in));
    CHK(dalloc(h, &h->c_seed, (size_t)B * h->J * (h->S > 0 ? h->S : 1)));
    if (h->cfg.variant == 5) CHK(dalloc(h, &h->c_seed_last, (size_t)B * h->J * h->S));      // (guidance: rows [B/2, B) = the twins' copy)
    CHK(dalloc(h, &h->c_audio, (size_t)B * h->Ta * h->As));
    CHK(dalloc(h, &h->mask, (size_t)B * h->T));
    CHK(dalloc(h, &h->ctr, 8));
    CHK(dalloc(h, &h->cfg_scale, (size_t)B));
    CHK(dalloc(h, &h->dyn, GemmArgs::dyn_words(B)));      // the noise block (GemmArgs::dyn)
    h->dyn_host.assign(GemmArgs::dyn_words(B), 0u);
    CHK(dalloc(h, &h->t_arr, (size_t)B));
    // the xs32 master is read as a GEMM operand in fp32 mode: rows padded to a 16-row tile exist (allocated above)
    return 0;
}

extern "C" int dsg_destroy(dsg_handle* h) {
    if (!h) return 0;
    CHK(owned_by_queue(h));
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& kv : h->graphs) { (void)hipGraphExecDestroy(kv.second.exec); (void)hipGraphDestroy(kv.second.graph); }
#ifndef DSG_EMU
    dsg_aql::destroy(h->aql);
#endif
    for (void* p : h->allocs) (void)hipFree(p);
    for (void* p : h->allocs_uc) uc_pool_give(h->cfg.device, p);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->ev_t0) (void)hipEventDestroy(h->ev_t0);
    if (h->ev_t1) (void)hipEventDestroy(h->ev_t1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

// A second sampling lane over the same weights: own stream / HSA queue, state, activations, conditioning and schedule, but
// the checkpoint-derived buffers (packed weights, time-embedding and rotary tables) are the source's, reference counted.
// `max_batch` <= 0 keeps the source's.
extern "C" int dsg_clone(dsg_handle* src, int max_batch, dsg_handle** out) {
    if (!src || !out) return fail(DSG_E_INVALID, "dsg_clone: null argument");
    if (!src->finalized) return fail(DSG_E_STATE, "dsg_clone before dsg_finalize_weights");
    dsg_config c = src->cfg;
    if (max_batch > 0) c.max_batch = max_batch;
    dsg_handle* h = nullptr;
    CHK(dsg_create(&c, &h));
    h->shared = src->shared;
    h->is_clone = true;
    h->raw = src->raw;
    h->Wp_in = src->Wp_in; h->Wp_out = src->Wp_out; h->b_out = src->b_out; h->layers = src->layers;
    h->TE = src->TE; h->TE2 = src->TE2; h->rcos = src->rcos; h->rsin = src->rsin; h->cbase = src->cbase;
    h->zero_bias = src->zero_bias;
    h->kset_req = src->kset_req;
    h->finalized = true;
    *out = h;
    return 0;
}

extern "C" int dsg_load_tensor(dsg_handle* h, const char* name, const void* data, const int64_t* shape, int ndim,
                               int dtype) {
    if (!h || !name || !data || !shape) return fail(DSG_E_INVALID, "dsg_load_tensor: null argument");
    CHK(owned_by_queue(h));
    if (h->is_clone) return fail(DSG_E_STATE, "dsg_load_tensor on a clone: load the weights into the source handle");
    if (dtype != 0) return fail(DSG_E_NOT_IMPLEMENTED, "dsg_load_tensor: only float32 (dtype 0)");
    HIPCHK(hipSetDevice(h->cfg.device));
    std::string nm(name);
    if (nm == "embed_timestep.sequence_pos_encoder.pe") nm = "sequence_pos_encoder.pe";   // aliased buffer
    auto exp = expected_tensors(h);
    auto it = exp.find(nm);
    if (it == exp.end()) return fail(DSG_E_UNEXPECTED_KEY, "unexpected key in state_dict: " + nm);
    size_t n = 1, ne = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    for (auto v : it->second) ne *= (size_t)v;
    bool same = (int)it->second.size() == ndim;
    for (int i = 0; same && i < ndim; ++i) same = it->second[i] == shape[i];
    if (!same || n != ne) return fail(DSG_E_INVALID, "size mismatch for " + nm);
    RawT& r = h->raw[nm];
    if (!r.d) {
        h->alloc_shared = true;
        const int rc = dalloc(h, &r.d, n, false);
        h->alloc_shared = false;
        CHK(rc);
    }
    r.n = n; r.shape.assign(shape, shape + ndim);
    const bool dev_src = is_device_ptr(data);
    HIPCHK(hipMemcpy(r.d, data, n * sizeof(float), dev_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    // a device-to-device hipMemcpy may return before the copy has run (null stream); the packing kernels that read r.d
    // run on the handle's non-blocking stream, which is not ordered against it
    if (dev_src) HIPCHK(hipDeviceSynchronize());
    h->finalized = false;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------------------
static int launch_mm(dsg_handle* h, float* C, int ldc, const float* A, long long sam, long long sak, const float* Bm,
                     long long sbn, long long sbk, const float* bias, const float* add, long long sadd, int add_div,
                     int M, int N, int K, int act = 0) {
    MMArgs a;
    a.C = C; a.ldc = ldc; a.A = A; a.sam = sam; a.sak = sak; a.Bm = Bm; a.sbn = sbn; a.sbk = sbk; a.bias = bias;
    a.add = add; a.sadd = sadd; a.add_div = add_div < 1 ? 1 : add_div; a.M = M; a.N = N; a.K = K; a.act = act;
    const size_t n = (size_t)M * N;
    if (n == 0) return 0;
    if (K >= 512 && n <= (1u << 20)) {  // long reductions: a wave per (row, 4 columns) (k_mm_wave); the big set-up tables stay on k_mm_naive
        const size_t nw = (size_t)M * ((N + 3) / 4);
        hipLaunchKernelGGL(k_mm_wave, dim3((int)std::min<size_t>((nw + 3) / 4, 16384)), dim3(256), 0, h->stream, a);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int grid = (int)std::min<size_t>((n + 127) / 128, 4096);
    hipLaunchKernelGGL(k_mm_naive, dim3(grid), dim3(128), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class P>
static int launch_pack(dsg_handle* h, void** dst, const float* W, long long ldw, int N, int K, int NT, int KBtot) {
    const size_t n = (size_t)NT * KBtot * 64 * P::E;
    CHK(dalloc_bytes(h, dst, n * sizeof(typename P::elem) * P::WF));
    const int grid = (int)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL((k_pack_w<P>), dim3(grid), dim3(256), 0, h->stream, *dst, W, ldw, N, K, NT, KBtot);
    HIPCHK(hipGetLastError());
    return 0;
}
static int pack(dsg_handle* h, void** dst, const float* W, long long ldw, int N, int K, int Npad, int Kpad) {
    if (h->prec == DSG_PREC_BF16) return launch_pack<PBF16>(h, dst, W, ldw, N, K, Npad / 16, Kpad / 32);
    if (h->prec == DSG_PREC_BF16W2) return launch_pack<PBF16W2>(h, dst, W, ldw, N, K, Npad / 16, Kpad / 32);
    return launch_pack<PF32>(h, dst, W, ldw, N, K, Npad / 16, Kpad / 16);
}
static int padded_vec(dsg_handle* h, float** dst, const float* src, int n, int npad) {
    CHK(dalloc(h, dst, (size_t)npad));
    hipLaunchKernelGGL(k_copy_pad, dim3(cdiv(npad, 256)), dim3(256), 0, h->stream, *dst, src, n, npad);
    HIPCHK(hipGetLastError());
    return 0;
}

static int finalize_weights(dsg_handle* h);
extern "C" int dsg_finalize_weights(dsg_handle* h) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    CHK(owned_by_queue(h));
    if (h->is_clone) return fail(DSG_E_STATE, "dsg_finalize_weights on a clone");
    h->alloc_shared = true;
    const int rc = finalize_weights(h);
    h->alloc_shared = false;
    return rc;
}
static int finalize_weights(dsg_handle* h) {
    HIPCHK(hipSetDevice(h->cfg.device));
    auto exp = expected_tensors(h);
    for (auto& kv : exp)
        if (!h->raw.count(kv.first)) return fail(DSG_E_MISSING_KEY, "missing key in state_dict: " + kv.first);
    auto R = [&](const std::string& n) { return h->raw[n].d; };
    const int D = h->D, J = h->J, A = h->A, ff = h->ff, L = h->L;
    const int W2ld = 2 * D + A;
    const float* W2 = R("input_process2.weight");

    // time-embedding tables  (TimestepEmbedder, main/model/mdm.py:434-448)
    float* H1 = nullptr;
    CHK(dalloc(h, &H1, (size_t)h->n_te * D));
    CHK(dalloc(h, &h->TE, (size_t)h->n_te * D));
    CHK(dalloc(h, &h->TE2, (size_t)h->n_te * D));
    CHK(launch_mm(h, H1, D, R("sequence_pos_encoder.pe"), D, 1, R("embed_timestep.time_embed.0.weight"), D, 1,
                  R("embed_timestep.time_embed.0.bias"), nullptr, 0, 1, h->n_te, D, D, 1));
    CHK(launch_mm(h, h->TE, D, H1, D, 1, R("embed_timestep.time_embed.2.weight"), D, 1,
                  R("embed_timestep.time_embed.2.bias"), nullptr, 0, 1, h->n_te, D, D, 0));
    CHK(launch_mm(h, h->TE2, D, h->TE, D, 1, W2, W2ld, 1, nullptr, nullptr, 0, 1, h->n_te, D, D, 0));
    // fold input_process2[:, D:2D] . poseEmbedding   (mdm.py:198, :202-206) -> [D][J]
    float* Wfold = nullptr;
    CHK(dalloc(h, &Wfold, (size_t)D * J));
    CHK(launch_mm(h, Wfold, J, W2 + D, W2ld, 1, R("input_process.poseEmbedding.weight"), 1, J, nullptr, nullptr, 0, 1,
                  D, J, D, 0));
    CHK(dalloc(h, &h->cbase, (size_t)D));
    CHK(launch_mm(h, h->cbase, D, R("input_process.poseEmbedding.bias"), 0, 1, W2 + D, W2ld, 1,
                  R("input_process2.bias"), nullptr, 0, 1, 1, D, D, 0));
    CHK(pack(h, &h->Wp_in, Wfold, J, D, J, D, h->Jp));
    CHK(dalloc(h, &h->zero_bias, (size_t)std::max(D, h->Jp)));
    for (int i = 0; i < L; ++i) {
        const std::string p = "seqTransEncoder.layers." + std::to_string(i) + ".";
        Layer& l = h->layers[i];
        CHK(pack(h, &l.Wqkv, R(p + "self_attn.in_proj_weight"), D, 3 * D, D, 3 * D, D));
        CHK(pack(h, &l.Wo, R(p + "self_attn.out_proj.weight"), D, D, D, D, D));
        CHK(pack(h, &l.W1, R(p + "linear1.weight"), D, ff, D, ff, D));
        CHK(pack(h, &l.W2, R(p + "linear2.weight"), ff, D, ff, D, ff));
        l.bqkv = R(p + "self_attn.in_proj_bias"); l.bo = R(p + "self_attn.out_proj.bias");
        l.b1 = R(p + "linear1.bias"); l.b2 = R(p + "linear2.bias");
        l.g1 = R(p + "norm1.weight"); l.be1 = R(p + "norm1.bias");
        l.g2 = R(p + "norm2.weight"); l.be2 = R(p + "norm2.bias");
    }
    CHK(pack(h, &h->Wp_out, R("output_process.poseFinal.weight"), D, J, D, h->Jp, D));
    CHK(padded_vec(h, &h->b_out, R("output_process.poseFinal.bias"), J, h->Jp));

    // rotary tables (rotary.py:12-16): freqs = pos * inv_freq in fp32, cos/sin of that fp32 value
    {
        const int half = h->hdl / 2, npos = h->T + 1;
        std::vector<float> inv(half), c((size_t)npos * half), s((size_t)npos * half);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(inv.data(), R("rel_pos.inv_freq"), half * sizeof(float), hipMemcpyDeviceToHost));
        for (int p = 0; p < npos; ++p)
            for (int k = 0; k < half; ++k) {
                const float fr = (float)p * inv[k];
                c[(size_t)p * half + k] = (float)std::cos((double)fr);
                s[(size_t)p * half + k] = (float)std::sin((double)fr);
            }
        CHK(dalloc(h, &h->rcos, c.size()));
        CHK(dalloc(h, &h->rsin, s.size()));
        HIPCHK(hipMemcpy(h->rcos, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->rsin, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->finalized = true;
    return 0;
}

extern "C" int dsg_set_schedule(dsg_handle* h, const double* betas, const int64_t* tmap, int n) {
    if (!h || !betas || !tmap) return fail(DSG_E_INVALID, "dsg_set_schedule: null argument");
    CHK(owned_by_queue(h));
    Sched s;
    CHK(build_sched(betas, n, s));
    s.tmap.resize(n);
    for (int i = 0; i < n; ++i) {
        if (tmap[i] < 0 || tmap[i] >= h->n_te) return fail(DSG_E_INVALID, "timestep_map entry out of range");
        s.tmap[i] = (int)tmap[i];
    }
    h->sched = s;
    h->st_valid = false;
    // captured graphs carry the table pointers and the table length of the schedule they were captured under
    for (auto& kv : h->graphs) { (void)hipGraphExecDestroy(kv.second.exec); (void)hipGraphDestroy(kv.second.graph); }
    h->graphs.clear();
    if (n > h->st_cap) {
        HIPCHK(hipSetDevice(h->cfg.device));
        CHK(dalloc(h, &h->st_tmodel, (size_t)n));
        for (int k = 0; k < 5; ++k) CHK(dalloc(h, &h->st_c[k], (size_t)n));
        h->st_cap = n;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// per-window conditioning (mdm.py:180-190; BEAT-TWH mdm.py:145, :188-190): everything that does not depend on x_t or t
// ---------------------------------------------------------------------------------------------------------
static int upload(dsg_handle* h, void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return 0;
}

static int order_after(dsg_handle* h, void* user_stream);
static int order_before(dsg_handle* h, void* user_stream);

// y['seed_last'] of DiffuseStyleGesture++ (cross_local_attention5, BEAT-TWH-main/model/mdm.py:229): [B, J, 1, S].  It is the same
// snippet for every window of a clip (BEAT-TWH sample.py:85-93), so it is handed over once and kept.
extern "C" int dsg_set_seed_last(dsg_handle* h, const float* seed_last, int B, void* stream) {
    if (!h || !seed_last) return fail(DSG_E_INVALID, "null argument");
    CHK(owned_by_queue(h));
    if (h->cfg.variant != 5) return fail(DSG_E_INVALID, "dsg_set_seed_last is for variant 5 (cross_local_attention5) only");
    if (B <= 0 || B > h->Bmax) return fail(DSG_E_INVALID, "batch exceeds max_batch");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(order_after(h, stream));
    CHK(upload(h, h->c_seed_last, seed_last, (size_t)B * h->J * h->S * sizeof(float)));
    h->seed_last_B = B;
    CHK(order_before(h, stream));     // the caller may release / overwrite its tensor once its stream has passed this point
    return 0;
}

// conditioning of batch rows [row0, row0 + B): inputs are the caller's B elements, `uncond` selects the masked variant
static int cond_rows(dsg_handle* h, const float* style, const float* seed, const float* audio, int row0, int B, int uncond) {
    auto R = [&](const std::string& n) { return h->raw[n].d; };
    const int D = h->D, J = h->J, S = h->S, A = h->A, As = h->As, T = h->T, sdi = h->cfg.style_dim_in;
    const int W2ld = 2 * D + A;
    const float* W2 = R("input_process2.weight");
    float* c_style = h->c_style + (size_t)row0 * sdi;
    float* c_seed = h->c_seed + (size_t)row0 * J * (S > 0 ? S : 1);
    float* c_audio = h->c_audio + (size_t)row0 * h->Ta * As;
    float* emb1 = h->emb1 + (size_t)row0 * D;
    float* enc = h->enc + (size_t)row0 * T * A;
    float* cvec = h->cvec + (size_t)row0 * D;
    float* Cf = h->Cf + (size_t)row0 * T * D;
    CHK(upload(h, c_style, style, (size_t)B * sdi * sizeof(float)));
    if (S > 0 && seed != c_seed) CHK(upload(h, c_seed, seed, (size_t)B * J * S * sizeof(float)));      // (dsg_sample_clip: k_window_handoff wrote it in place)
    CHK(upload(h, c_audio, audio, (size_t)B * h->Ta * As * sizeof(float)));
    const int sdo = h->cfg.variant == 3 ? 64 : D;
    if (uncond) {       // mask_cond(force_mask=True): zeros AFTER the style linear (mdm.py:156-159, :180)
        hipLaunchKernelGGL(k_fill_f32, dim3(cdiv(B * D, 256)), dim3(256), 0, h->stream, emb1, 0.f, (size_t)B * D);
        HIPCHK(hipGetLastError());
    } else {
        CHK(launch_mm(h, emb1, D, c_style, sdi, 1, R("embed_style.weight"), sdi, 1, R("embed_style.bias"),
                      nullptr, 0, 1, B, sdo, sdi));
    }
    if (h->cfg.variant == 3) {
        // embed_text(flattened seed) -> emb1[:, 64:]; with force_mask the seed is zeroed BEFORE the linear (bias only)
        CHK(launch_mm(h, emb1 + 64, D, c_seed, (long long)J * S, 1, R("embed_text.weight"), (long long)J * S, 1,
                      R("embed_text.bias"), nullptr, 0, 1, B, D - 64, uncond ? 0 : J * S));
        CHK(launch_mm(h, enc, A, c_audio, As, 1, R("WavEncoder.audio_feature_map.weight"), As, 1,
                      R("WavEncoder.audio_feature_map.bias"), nullptr, 0, 1, B * T, A, As));
    } else {
        for (int b = 0; b < B; ++b) {
            // per-frame seed embedding: rows 0..S-1 of the "audio" block  (BEAT-TWH mdm.py:188)
            CHK(launch_mm(h, enc + (size_t)b * T * A, A, c_seed + (size_t)b * J * S, 1, S, R("embed_text.weight"),
                          J, 1, R("embed_text.bias"), nullptr, 0, 1, S, A, J));
            CHK(launch_mm(h, enc + ((size_t)b * T + S) * A, A, c_audio + (size_t)b * h->Ta * As, As, 1,
                          R("WavEncoder.audio_feature_map.weight"), As, 1, R("WavEncoder.audio_feature_map.bias"),
                          nullptr, 0, 1, h->Ta, A, As));
            if (h->cfg.variant == 5)    // rows S+Ta .. T-1: embed_text_last(y['seed_last'])  (BEAT-TWH mdm.py:229-230)
                CHK(launch_mm(h, enc + ((size_t)b * T + S + h->Ta) * A, A, h->c_seed_last + (size_t)(row0 + b) * J * S, 1, S,
                              R("embed_text_last.weight"), J, 1, R("embed_text_last.bias"), nullptr, 0, 1, S, A, J));
        }
    }
    // cvec[b] = b2 + W2b.bp + W2a.emb1[b];  Cf[b,f] = W2c.enc[b,f] + cvec[b]
    CHK(launch_mm(h, cvec, D, emb1, D, 1, W2, W2ld, 1, nullptr, h->cbase, 0, 1, B, D, D));
    CHK(launch_mm(h, Cf, D, enc, A, 1, W2 + 2 * D, W2ld, 1, nullptr, cvec, D, T, B * T, D, A));
    return 0;
}

// cfg_scale == nullptr: plain conditioning (`uncond` as given).  Else classifier-free guidance: rows [0, B) conditional,
// rows [B, 2B) their unconditional twins, guidance scale per element (y['scale'], cfg_sampler.py:29-31).
static int set_window_cond(dsg_handle* h, const float* style, const float* seed, const float* audio,
                           const uint8_t* mask_local, int mask_batch, int B, int uncond, const float* cfg_scale, void* stream) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    if (!h->finalized) return fail(DSG_E_STATE, "dsg_set_window_cond before dsg_finalize_weights");
    const int rows = cfg_scale ? 2 * B : B;
    if (B <= 0 || rows > h->Bmax) return fail(DSG_E_INVALID, cfg_scale ? "classifier-free guidance needs max_batch >= 2 * batch" : "batch exceeds max_batch");
    if (!style || !audio || (h->S > 0 && !seed)) return fail(DSG_E_INVALID, "style/seed/audio required");
    if (mask_local && !(mask_batch >= 1 && (B * h->Hl) % mask_batch == 0))
        return fail(DSG_E_INVALID, "mask_local batch must divide B*heads");
    if (h->cfg.variant == 5 && h->seed_last_B != B)
        return fail(DSG_E_STATE, "variant 5: call dsg_set_seed_last with the same batch before dsg_set_window_cond (y['seed_last'])");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(order_after(h, stream));      // the caller's stream may still be producing seed / audio
    const int T = h->T;
    if (mask_local) {
        CHK(upload(h, h->mask, mask_local, (size_t)mask_batch * T));
        h->mb = mask_batch;
        if (cfg_scale && mask_batch > 1) {          // the twins use the same key masks: rows [B, 2B) repeat rows [0, B)
            if (mask_batch != B) return fail(DSG_E_NOT_IMPLEMENTED, "guidance: mask_local batch must be 1 or B");
            CHK(upload(h, h->mask + (size_t)B * T, mask_local, (size_t)B * T));
            h->mb = 2 * B;
        }
        h->nomask = 0;
    } else {
        // `mask=None` (local_attention.py:196-210 skipped): only the causal mask applies and the look-back pads of window 0
        // attend with key = value = -1
        HIPCHK(hipMemsetAsync(h->mask, 1, (size_t)T, h->stream));
        h->mb = 1;
        h->nomask = 1;
    }
    CHK(cond_rows(h, style, seed, audio, 0, B, cfg_scale ? 0 : uncond));
    if (cfg_scale) {
        if (h->cfg.variant == 5)      // the twins see the same closing snippet
            HIPCHK(hipMemcpyAsync(h->c_seed_last + (size_t)B * h->J * h->S, h->c_seed_last, (size_t)B * h->J * h->S * sizeof(float),
                                  hipMemcpyDeviceToDevice, h->stream));
        CHK(cond_rows(h, style, seed, audio, B, B, 1));
        CHK(upload(h, h->cfg_scale, cfg_scale, (size_t)B * sizeof(float)));
    }
    h->cfgB = cfg_scale ? B : 0;
    h->cond_set = true;
    h->condB = rows;
    CHK(order_before(h, stream));     // uploads are enqueued copies: the caller's buffers are free once its stream passes this point
    return 0;
}
extern "C" int dsg_set_window_cond(dsg_handle* h, const float* style, const float* seed, const float* audio,
                                   const uint8_t* mask_local, int mask_batch, int B, int uncond, void* stream) {
    CHK(owned_by_queue(h));
    return set_window_cond(h, style, seed, audio, mask_local, mask_batch, B, uncond, nullptr, stream);
}
extern "C" int dsg_set_window_cond_cfg(dsg_handle* h, const float* style, const float* seed, const float* audio,
                                       const uint8_t* mask_local, int mask_batch, int B, const float* scale, void* stream) {
    CHK(owned_by_queue(h));
    if (!scale) return fail(DSG_E_INVALID, "dsg_set_window_cond_cfg: scale required (y['scale'])");
    return set_window_cond(h, style, seed, audio, mask_local, mask_batch, B, 0, scale, stream);
}

// ---------------------------------------------------------------------------------------------------------
// Kernel sets.  ONE function decides which kernels a step of B batch rows runs (select_kernels); nothing else in this file
// looks at sizes.  A set is a property of the handle (dsg_set_kernel_set) or, with DSG_KSET_AUTO, a function of the batch
// alone -- never of how many lanes happen to run together -- so the same (handle, batch, seed) gives the same bits whether
// it is sampled by dsg_sample or as one lane of dsg_sample_multi.  What the sets are and the measurements behind the
// automatic rule (MI355X, ZEGGS dims, bf16; profiles/r02_u_kernel_sets.log, r02_i_lanes.log, r02_c_blk_sweep.log):
//
//   set      kernels of one step                                                  dispatches   wins at
//   LATENCY  k_inloc, L x {QKV 16x16, k_attn_mid | k_attn + k_mid, linear2}, head   2 + 3L      one lane, batch <= 2: 106.7 us vs
//                                                                                               122.0 (no k_attn_mid) / 125.5 (TILE)
//   TILE     k_in, k_loc, L x {QKV, k_attn_op | k_attn + out_proj, linear1,          3 + 4L      batch 3 .. 11 (182 vs 187 us at 3,
//            linear2} on 16 x 16 tiles (LayerNorm GEMMs "lean" from 512 rows), head              195 vs 197 at 4, 227 vs 235 at 8)
//   BLOCK    the same with 32-row block GEMMs for QKV / linear1 / linear2 / embedding 3 + 4L      >= 1000 rows in one lane (254 vs 293
//            (dsg_batched.h); out_proj and the pose head stay on 16 x 16 tiles                    us at 16); from 300 rows per lane when
//                                                                                               several lanes share the CUs (4 x 4:
//                                                                                               4691 vs 4400 frames/s, 4 x 16: 8243 vs 6447)
//   STREAM   weight-stationary persistent GEMMs for every K = D / K = ff product of a layer      3 + 5L      >= 2800 rows in one lane (batch 32: 372 ->
//            (dsg_stream.h: W panel in registers, activations global -> LDS, 32x32x16 MFMA):                357 us, batch 64: 611 -> 505); >= 1400 rows per
//            LayerNorm once per row (k_ln_frag), QKV, linear1, linear2, pose head; pose embedding         lane with several lanes (4 x 16: 10.2k -> 11.7k
//            and layer-0 QKV as in BLOCK                                                                  frames/s, 4 x 32: 11.0k -> 13.3k); slower below
//                                                                                                         (4 x 8: 8.3k vs 8.8k, batch 16: 316 vs 240 us)
//   With several lanes sharing the GPU the redundant recompute of LATENCY costs from batch 2 (4 x 2: 3507 frames/s TILE vs
//   3303 LATENCY): dsg_recommend_kernel_set(B, lanes) encodes the multi-lane column; the caller applies it to its lanes.
//   k_attn_op (attention + out_proj + LayerNorm1 in one kernel) replaces k_attn + out_proj in TILE / BLOCK wherever an
//   instantiation exists (bf16, Core::C256 / C128 = ZEGGS / tiny dims): 1 x 16: 292 -> 254 us, 4 x 4: 4640 -> 5074 frames/s.  Within a set
//   nothing depends on the batch but the grid (and the register budget of the LayerNorm GEMMs from 512 rows, same arithmetic):
//   a row's result is bit-identical whatever the batch it rides in.
// ---------------------------------------------------------------------------------------------------------
// A layer form names ONE fixed kernel sequence of an encoder layer (layer_<form> below).  select_kernels picks the form of every
// layer; fused guidance swaps the last layer's (layer_form).  A form whose feed-forward ends in k_ffn / k_ffn_ln leaves LayerNorm2
// of its rows fragment-major in X0a; the others leave pre2, which the next QKV projection / the pose head normalise on read.
enum class Form {
    MID,            // QKV, [k_attn], k_mid | k_attn_mid, linear2                       LATENCY
    UNFUSED,        // QKV, k_attn, out_proj, LayerNorm1 + linear1, linear2              TILE / BLOCK without k_attn_op
    ATTN_OP,        // QKV, k_attn_op[_w], linear1, linear2                             TILE / BLOCK with k_attn_op; the last layer under fused guidance
    ATTN_OP_SPLIT,  // QKV, k_attn_op[_w], k_ffn_part, k_ffn_ln                         BLOCK: C384 / C512 (bf16), C256 in fp32, DSG_CLIP_ATTN=0
    CLIP_SPLIT,     // k_clip_attn, k_ffn_part<OP>, k_ffn_ln                            BLOCK, bf16 at C256 / C128
    ATTN_OP_FFN,    // QKV, k_attn_op, k_ffn                                            STREAM / ROWS under DSG_CLIP_ATTN=0
    CLIP_FFN,       // k_clip_attn, k_ffn<OP>                                           STREAM, ROWS (bf16, bf16w2) at C256 / C128
    CLIP_W_FFN,     // k_clip_attn_w, k_ffn<OP>                                         ROWS at C384 / C512
    QKV_ATTN_FFN,   // QKV (on the hi + lo rows in X0a), k_attn, k_ffn<OP>              ROWS at C384 / C512 in bf16w2
};
static bool leaves_x0a(Form f) { return f >= Form::ATTN_OP_SPLIT; }
struct KernelSel {
    int set = DSG_KSET_TILE;
    Form form = Form::UNFUSED;
    bool attn_in_mid = false;   // MID: the attention inside k_mid (batch 1)
    int ffn_rows = 0;           // *_FFN: token rows per k_ffn workgroup, 16 / 32 / 64 (bit-identical whatever the block: the same waves, the same k order)
    bool xs_frag = false;       // BLOCK / STREAM / ROWS (bf16): the state shadow is fragment-major and the pose embedding streams it (k_ws2<EPI_PARTIAL>:
                                // 8.9 -> 4.3 us at 1424 rows, 29.9 -> 11.0 at 5632; 3.8 -> 4.1 at 356)
    int x0a_frag = 0;           // the layout k_loc leaves the embedding rows in (X0a): 0 row-major, 1 fragment-major, 2 ... as a hi + lo bf16 pair
    int ks_in = 1;              // workgroup split-K of the pose embedding
    bool blk() const { return set >= DSG_KSET_BLOCK; }       // 32-row block GEMMs (STREAM / ROWS: pose embedding and layer-0 QKV as in BLOCK)
    bool stream() const { return set == DSG_KSET_STREAM; }   // weight-stationary streaming GEMMs (dsg_stream.h)
};
static bool have_attn_mid(const dsg_handle* h, int B) {
    return B == 1 && core_narrow(h);
}
// The predicates below are the supported-shape matrix: (precision, Core) -- named in classify_core -- plus ff_size / the padded pose width where a form needs them.
// k_attn_op with all of W_o in registers: bf16 at C256 / C128 (the STREAM set builds on it)
static bool have_attn_op_narrow(const dsg_handle* h) {
    return h->prec == DSG_PREC_BF16 && core_narrow(h);
}
// ... or k_attn_op_w (W_o streamed in chunks, round 4): C384 / C512 in bf16, C256 / C128 in fp32
static bool have_attn_op_wide(const dsg_handle* h) {
    if (h->prec == DSG_PREC_BF16) return core_wide(h);
    return h->prec == DSG_PREC_FP32 && core_narrow(h);
}
static bool have_attn_op(const dsg_handle* h) { return have_attn_op_narrow(h) || have_attn_op_wide(h); }
static bool latency_set_ok(const dsg_handle* h) {
    // k_mid pulls all of W_o (2 D^2 bytes) through every CU: at D = 512 the un-fused sets win (TWH: 219 vs 238 us)
    // and at D = 384 with the K = D GEMMs in one fragment batch (round 4): BEAT 163.9 (TILE) vs 175-179 us (LATENCY) at batch 1
    // (profiles/r04_b_timeline_beat_tile_ch12.json, r04_a_timeline_beat_latency.json).  An explicit dsg_set_kernel_set(LATENCY) still
    // runs k_mid at every width <= 512.
    const int dt = h->D / 64;
    return h->D <= 256 && (dt == 1 || dt == 2 || dt == 4);
}
static bool stream_set_ok(const dsg_handle* h) {
    // k_ws keeps 64 columns x K = D of W per wave in registers (C128 / C256), k_ws2 a quarter of K = ff (ff = 128 / 1024);
    // linear1 reads the fragment-major LayerNorm1 rows k_attn_op writes
    return have_attn_op_narrow(h) && (h->ff == 1024 || h->ff == 128) && (h->Jp == 1152 || h->Jp == 128);
}
// k_ffn_part + k_ffn_ln exist for the shapes the STREAM set exists for and (round 5) for the DSG+ widths in bf16 (latent_dim 384 / 512, ff 1024:
// 8 ff-splits -- the two-batch weight fragments of these widths do not fit 4), behind k_attn_op_w
static bool ffn_split_wide(const dsg_handle* h) {
    if (h->prec == DSG_PREC_FP32) return h->core == Core::C256 && h->ff == 1024;      // (fp32, ZEGGS widths: K = 256 is 16 k-blocks of 16)
    return h->prec == DSG_PREC_BF16 && core_wide(h) && h->ff == 1024;
}
static bool ffn_split_ok(const dsg_handle* h) { return stream_set_ok(h) || ffn_split_wide(h); }
// ROWS at the DSG+ widths (round 6, bf16): k_clip_attn_w (dsg_stream.h: the clip's rows do not fit the LDS next to Q / K / V -- they pass through it in chunks; first
// version: the direct QKV GEMM + k_attn) feeds k_ffn<OP> on one 16-row tile (out_proj + LayerNorm1 as its prologue): no k_attn_op_w, no ff-split, no slabs, no slab-sum
// pass; streamed pose embedding (K over two workgroups) and pose head
static bool rows_wide_ok(const dsg_handle* h) {
    return h->prec == DSG_PREC_BF16 && core_wide(h) && h->ff == 1024;
}
// bf16w2 (round 6): the ROWS pair -- k_clip_attn + k_ffn on one 16-row tile -- exists with the two-register fragments at the ZEGGS / tiny widths
// (not under fused guidance: its last layer runs the QKV GEMM + k_attn_op, which have no bf16w2 form)
static bool rows_w2_ok(const dsg_handle* h) {
    return h->prec == DSG_PREC_BF16W2 && ((h->core == Core::C256 && h->ff == 1024) || (h->core == Core::C128 && h->ff == 128));
}
// bf16w2 at the DSG+ widths: the decomposition rows_wide_ok started from -- the direct QKV GEMM (k_gemm_qkv_pair: its rows are the hi + lo pair in X0a) + k_attn,
// then k_ffn<OP> on one 16-row tile with W_o leading a 16-slot ring of two-register fragments and the operand fragments re-read from LDS (A_LDS): 3 + 3L
// dispatches; 16 x 16 tile pose embedding and pose head.  Reachable by name only: resolve_auto_set and the uc_mode decision of dsg_create read rows_w2_ok, not this
static bool rows_w2_wide_ok(const dsg_handle* h) {
    return h->prec == DSG_PREC_BF16W2 && core_wide(h) && h->ff == 1024;
}
// the streamed pose embedding at the DSG+ pose widths (round 6: k_ws2<EPI_PARTIAL, 17 / 18, 2>, K over two workgroups) -- in the ROWS set
// (a GEMM of K = Jp, N = latent_dim: it depends on those two widths alone, not on the attention core -- any head count / clip length)
static bool xs_frag_wide(const dsg_handle* h, int set) {
    return (set == DSG_KSET_ROWS || set == DSG_KSET_BLOCK) && (h->Jp == 2176 || h->Jp == 2304) && (h->D == 384 || h->D == 512);
}
static int auto_kernel_set(const dsg_handle* h, int B, int lanes) {
    const int rows = B * h->ntok, MT = cdiv(rows, 16);
    const bool s_ok = stream_set_ok(h);       // (bf16, the ZEGGS / tiny widths: STREAM and ROWS exist)
    // Round 6 (one-box sweeps of every set, us per step; profiles/r06_u_*, r06_v_*, r06_w_* before, r06_cb_sweep_rows_gradual.log after the ring's first fill
    // was spread over LayerNorm1): ROWS -- k_ffn on one 16-row tile per workgroup -- wins wherever the row tiles of ALL lanes fit the 256 CUs in one round:
    // 1 x 10 clips 183.0 vs 186.0 (BLOCK), 1 x 12: 184.3 vs 190.3, 1 x 16: 188.0 vs 204, 1 x 24: 203 vs 298 (BLOCK) / 249 (STREAM), 1 x 46 (256 row tiles):
    // 228.7 vs 237.8 (STREAM); 1 x 48 (267 tiles: two rounds): 320 vs 240 -> STREAM; 4 x 3: 184.6 vs 187.1 (BLOCK), 4 x 4: 186.8 vs 194.2, 4 x 5: 189.9 vs
    // 198.7, 2 x 8: 186.4 vs 189.9, 4 x 12 (268 tiles): 225.5 vs 230.4 (STREAM), 4 x 14 (312): 243.4 = 240.7, 4 x 16: 264 vs 250 -> STREAM; 2 x 24: 229 vs
    // 238, 2 x 32: 274 vs 249 -> STREAM.  Below ~900 token rows over all lanes BLOCK's ff-split is even or ahead (1 x 8: 181.9 vs 180.8, 1 x 6: 180.6 vs
    // 177.6, 1 x 5: 180.3 vs 176.4 -- TILE 161.6 --, 2 x 4: 180.5 vs 178.1, 2 x 6: 184.0 = 183.8; 4 x 2: 181.7 vs 183.3, TILE 179.4).
    // (rounds 4-5, STREAM against BLOCK: profiles/r04_n_sweep_sets.log, r05_j_sweep_sets.log)
    if (lanes <= 1) {
        if (s_ok && rows >= 800) return MT <= 256 ? DSG_KSET_ROWS : DSG_KSET_STREAM;
        // (fp32, round 5: k_attn_mid recomputes out_proj per hidden slice, and an fp32 MFMA is 1/16 of a bf16 one -- the un-fused 16 x 16
        // tiles win at batch 1: 208.2 vs 218.5 us per step, profiles/r05_g_bench_fp32_*.log)
        if (B <= 2 && latency_set_ok(h) && h->prec != DSG_PREC_FP32) return DSG_KSET_LATENCY;
        // (DSG+ widths, round 5: with k_ffn_part + k_ffn_ln behind k_attn_op_w BLOCK wins from 4 clips -- BEAT 283 vs 303 us, TWH 310 vs 365; 2 clips: 259 vs 198)
        // (only there: ffn_split_wide() is also true for fp32 at the ZEGGS widths, which has no such measurement -- round-5 advisor)
        // (round 6, DSG+ widths: ROWS -- direct QKV + k_attn + k_ffn<OP> on 16-row tiles -- from 9 clips while the row tiles fit the CUs in one round: BEAT 1 x 16
        //  526 -> 443 us per step, 1 x 24: 701 -> 556, 1 x 26: 806 -> 594, 1 x 8: 370 -> 346; TWH 1 x 16: 609 -> 524, 1 x 24: 835 -> 660, 1 x 8: 417 -> 410; below: BLOCK
        //  (BEAT 1 x 6: 297 vs 305, TWH 1 x 6: 326 vs 366) -- profiles/r06_da_*, r06_db_*)
        //  (... and past one round of the CUs as well: BEAT 1 x 32 clips 702 vs 844 us BLOCK, 1 x 48: 822 vs 1179; TWH 1 x 32: 925 vs 1058 -- profiles/r06_dm_*)
        //  (with k_clip_attn_w -- 24 us at latent_dim 512 whatever the batch -- BLOCK keeps 9 .. 12 TWH clips: 1 x 9: 417 vs 452 us, 1 x 12: 457 vs 466, 1 x 14: 551 vs 472;
        //   BEAT 1 x 9: 356 vs 339 ROWS -- profiles/r06_dv_*)
        if (rows_wide_ok(h) && h->cfgB == 0 && rows >= (h->core == Core::C512 ? 1960 : 1300)) return DSG_KSET_ROWS;
        if (ffn_split_wide(h) && h->prec == DSG_PREC_BF16 && h->env_ffn_split != 0 && rows >= 600) return DSG_KSET_BLOCK;
        // (round 6, bf16 ZEGGS widths: BLOCK from 6 clips -- 1 x 6: 177.6 vs 190.1 TILE, 1 x 5: 176.4 vs 161.6, 1 x 4: 173.9 vs 157.4)
        return rows >= (s_ok ? 500 : 1000) ? DSG_KSET_BLOCK : DSG_KSET_TILE;
    }
    if (s_ok && rows >= 850 && lanes * MT > 300) return DSG_KSET_STREAM;
    if (s_ok && rows >= 250 && lanes * rows >= 1000 && lanes * MT <= 300) return DSG_KSET_ROWS;
    // (DSG+ widths with several lanes: ROWS from 4 clips per lane and 16 over all lanes -- BEAT 4 x 4: 399 vs 405, 2 x 8: 412 vs 445, 4 x 8: 627 vs 699; TWH 4 x 4: 509 vs 518,
    //  2 x 8: 514 vs 549, 4 x 8: 794 vs 949; below: BLOCK -- 4 x 3: 342 vs 363, 2 x 4: 297 vs 304, 4 x 2: 297 vs 319)
    if (rows_wide_ok(h) && h->cfgB == 0 && rows >= 600 && lanes * rows >= 2400) return DSG_KSET_ROWS;
    if (B <= 1 && latency_set_ok(h) && h->prec != DSG_PREC_FP32) return DSG_KSET_LATENCY;
    // (2 x 4: BLOCK 178.1 vs ROWS 180.5; 4 x 2: TILE 179.4 vs BLOCK 183.3; 2 x 3: 175.1 = 173.8)
    return rows >= (s_ok ? 250 : 300) ? DSG_KSET_BLOCK : DSG_KSET_TILE;
}
// what DSG_KSET_AUTO resolves to for `lanes` lanes of batch B: the measured table + dsg_config.latency_mode (1 = never LATENCY, 2 = always
// where LATENCY is a sensible choice at all: latent_dim <= 256, see latency_set_ok).  ONE function for select_kernels and
// dsg_recommend_kernel_set (round-4 advisor: the two used to disagree at the DSG+ widths)
static int resolve_auto_set(const dsg_handle* h, int B, int lanes) {
    int set = auto_kernel_set(h, B, lanes);
    if (h->latency_mode == 0 && set == DSG_KSET_LATENCY) set = DSG_KSET_TILE;
    // bf16w2: 16 x 16 tiles at every batch size.  Its weight fragments are twice the bytes, so the redundant W_o of the fused LATENCY
    // kernels costs more than the dispatches it saves: 168 vs 155 us per batch-1 step (profiles/r05_e_*); LATENCY stays selectable
    // (round 6: ... and ROWS -- k_clip_attn + k_ffn with the two-register fragments -- from 800 token rows in one lane / 1400 over several lanes of >= 300:
    //  1 x 16 clips 331 vs 453 us per step, 4 x 4: 330 vs 348, 1 x 8: 315 vs 311, 1 x 4: 310 vs 208 -- profiles/r06_bb_w2_rows.log.  Every workgroup
    //  streams W_o + W1 + W2 as hi + lo pairs, 2.3 MB through one CU's 64 B / clk load path: k_ffn is 23.7 us whatever the batch, r06_bc_marks_b16_rows_w2.log)
    if (h->prec == DSG_PREC_BF16W2) {
        const int rows = B * h->ntok;
        const bool big = rows >= 800 || (lanes > 1 && rows >= 300 && lanes * rows >= 1400);
        set = (rows_w2_ok(h) && h->cfgB == 0 && big) ? DSG_KSET_ROWS : DSG_KSET_TILE;
    }
    if (h->latency_mode == 1 && latency_set_ok(h)) set = DSG_KSET_LATENCY;
    return set;
}
// whether the handle can run `set` (not AUTO) at all: dsg_set_kernel_set refuses what every later step would
static int check_set(const dsg_handle* h, int set) {
    if (set < DSG_KSET_LATENCY || set > DSG_KSET_ROWS) return fail(DSG_E_INVALID, "unknown kernel set");
    if (set == DSG_KSET_LATENCY && h->D > 512) return fail(DSG_E_NOT_IMPLEMENTED, "kernel set LATENCY: latent_dim > 512");
    if ((set == DSG_KSET_STREAM || set == DSG_KSET_ROWS) && !stream_set_ok(h) && !(set == DSG_KSET_ROWS && (rows_w2_ok(h) || rows_wide_ok(h) || rows_w2_wide_ok(h))))
        return fail(DSG_E_NOT_IMPLEMENTED, "kernel sets STREAM / ROWS: bf16, latent_dim 128 / 256, 4 heads, ff 128 / 1024 (ROWS: bf16w2 there as well, and bf16 / bf16w2 at the DSG+ widths -- latent_dim 384 / 512, ff 1024) only");
    if (h->prec == DSG_PREC_BF16W2 && ((set > DSG_KSET_TILE && !(set == DSG_KSET_ROWS && (rows_w2_ok(h) || rows_w2_wide_ok(h)))) || (set == DSG_KSET_LATENCY && h->D > 256)))
        return fail(DSG_E_NOT_IMPLEMENTED, "precision bf16w2: kernel sets LATENCY (latent_dim <= 256), TILE and ROWS (latent_dim 128 / 256, ff 128 / 1024; 384 / 512, ff 1024; 4 heads) only");
    return 0;
}
// lanes: how many lanes share the GPU in this call (RunMode::lanes) -- the block shape of k_ffn, never the set or the arithmetic
static int select_kernels(const dsg_handle* h, int B, int lanes, KernelSel& k) {
    int set = h->kset_req;
    if (set == DSG_KSET_AUTO) set = resolve_auto_set(h, B, 1);
    CHK(check_set(h, set));
    const bool w2 = h->prec == DSG_PREC_BF16W2;
    // (bf16w2: the guided last layer runs ATTN_OP, which has no bf16w2 form; at the DSG+ widths ROWS has its own guided pose head, k_ws_cfg)
    if (set == DSG_KSET_ROWS && h->cfgB > 0 && w2) return fail(DSG_E_NOT_IMPLEMENTED, "precision bf16w2, kernel set ROWS: no fused guidance (TILE has it)");
    k = KernelSel();
    k.set = set;
    const int rows = B * h->ntok, e = h->env_ffn_rt4;
    const bool clip = have_attn_op_narrow(h) && h->env_clip_attn != 0;      // (A/B: DSG_CLIP_ATTN=0 = QKV GEMM + k_attn_op, round 4)
    // k_ffn on 64-row blocks: 4 lanes x >= 4000 token rows (4 x 64 clips: 981 -> 903 us per step of the 4 lanes; 1 x 64: 376 -> 432, 4 x 16: 334 -> 392,
    // 4 x 32 even -- profiles/r04_y2_sweep_ffn_rt4_*.log).  DSG_FFN_RT4=<rows> (test hook / A/B): from that many token rows at any lane count; 0: never
    const bool rt4 = h->core == Core::C256 && (e >= 0 ? (e > 0 && rows >= e) : (lanes >= 4 && rows >= 4000));
    switch (set) {
        case DSG_KSET_LATENCY:
            k.form = Form::MID;
            k.attn_in_mid = have_attn_mid(h, B);
            break;
        case DSG_KSET_TILE:
            // (k_attn_op_w -- W_o streamed: DSG+ widths, fp32 -- belongs to BLOCK only: a set's arithmetic never depends on the batch, and at batch 1
            //  its 10 workgroups per layer lose to k_attn + out_proj -- BEAT: 200 vs 163 us/step; 16 clips: 3371 vs 2904 frames/s)
            k.form = have_attn_op_narrow(h) ? Form::ATTN_OP : Form::UNFUSED;
            break;
        case DSG_KSET_BLOCK:      // (A/B: DSG_FFN_SPLIT=0 = linear1 + linear2 + LayerNorm-on-read, round 3)
            if (ffn_split_ok(h) && h->env_ffn_split != 0) k.form = clip ? Form::CLIP_SPLIT : Form::ATTN_OP_SPLIT;
            else k.form = have_attn_op(h) ? Form::ATTN_OP : Form::UNFUSED;
            break;
        case DSG_KSET_STREAM:     // (round 4: k_ffn instead of k_ws<GELU> + k_ws2<RESID> + k_ln_frag)
            k.form = clip ? Form::CLIP_FFN : Form::ATTN_OP_FFN;
            k.ffn_rows = rt4 ? 64 : 32;
            break;
        default:
            // ROWS (round 6): BLOCK's first and last kernels around STREAM's per-layer pair, with k_ffn on ONE 16-row tile per workgroup -- no ff-split,
            // no partial slabs, no k_ffn_ln: 3 + 2L dispatches.  Every workgroup streams W_o + W1 + W2 (1.15 MB) for 16 rows, so it pays while the row
            // tiles of all lanes fit the 256 CUs in one round
            if (rows_wide_ok(h)) {      // (>= 3 lanes whose row tiles together exceed one round of the CUs: 32-row blocks, see layer_clip_w_ffn)
                k.form = Form::CLIP_W_FFN;
                k.ffn_rows = lanes >= 3 && lanes * cdiv(rows, 16) > 256 ? 32 : 16;
            } else if (rows_w2_wide_ok(h)) {      // (16-row tiles at every lane count: the only W2 block shape)
                k.form = Form::QKV_ATTN_FFN;
                k.ffn_rows = 16;
            } else if (w2 || clip) {
                k.form = Form::CLIP_FFN;
                k.ffn_rows = 16;
            } else {
                k.form = Form::ATTN_OP_FFN;
                k.ffn_rows = rt4 ? 64 : 32;
            }
    }
    k.xs_frag = k.blk() && h->prec == DSG_PREC_BF16 && (h->Jp == 1152 || h->Jp == 128 || xs_frag_wide(h, set));
    const bool clip_form = k.form == Form::CLIP_SPLIT || k.form == Form::CLIP_FFN || k.form == Form::CLIP_W_FFN;
    k.x0a_frag = (k.stream() || clip_form || k.form == Form::QKV_ATTN_FFN) ? (w2 ? 2 : 1) : 0;      // (QKV_ATTN_FFN: k_gemm_qkv_pair reads the pair)
    // split-K of the pose-embedding GEMM across workgroups: one split per 256 pose features for the 16 x 16 tile kernel; the block kernel splits K
    // over its 4 waves already, so 2 workgroup splits keep a wave's share at <= 8 k-blocks (one batch of loads) without fragmenting the work 5 ways.
    // (streamed embedding: K stays whole but at the DSG+ pose widths, see k_ws2; bf16w2: the 16 x 16 tiles)
    k.ks_in = k.xs_frag ? (h->Jp > 1152 ? 2 : 1) : ((k.blk() && !w2) ? std::min(h->KSin, 2) : h->KSin);
    return 0;
}
// fused guidance: the last layer leaves pre2 to the two-pass pose head k_gemm_cfg, which normalises on read -- where the set's form
// leaves X0a, that layer runs the round-3 feed-forward kernels behind k_attn_op instead.  CLIP_W_FFN (ROWS at the DSG+ widths, where no narrow k_attn_op
// exists) keeps its form: its guided pose head k_ws_cfg streams the conditional rows and their twins from X0a
static bool cfg_head_streams(Form f) { return f == Form::CLIP_W_FFN; }
static Form layer_form(const dsg_handle* h, const KernelSel& k, int l) {
    return h->cfgB > 0 && l == h->L - 1 && leaves_x0a(k.form) && !cfg_head_streams(k.form) ? Form::ATTN_OP : k.form;
}

// buffers only one kernel set needs, allocated when a call first runs that set (never inside a graph capture / packet recording:
// the callers invoke this right after select_kernels)
static int ensure_set_buffers(dsg_handle* h, const KernelSel& k) {
    if ((k.form == Form::ATTN_OP_SPLIT || k.form == Form::CLIP_SPLIT) && !h->ffn_part) {
        const bool was = h->alloc_uc;
        h->alloc_uc = true;
        const int rc = dalloc(h, &h->ffn_part, (size_t)(ffn_split_wide(h) ? 8 : 4) * h->ffn_slab);      // [S][M_pad][D] fp32, loop-written: uncached like the other activations
        h->alloc_uc = was;
        if (rc) return rc;
    }
    return 0;
}

extern "C" int dsg_set_kernel_set(dsg_handle* h, int set) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    CHK(owned_by_queue(h));
    if (set < DSG_KSET_AUTO || set > DSG_KSET_ROWS) return fail(DSG_E_INVALID, "dsg_set_kernel_set: unknown kernel set");
    if (set != DSG_KSET_AUTO) CHK(check_set(h, set));      // (round-5 advisor: this entry point used to accept LATENCY at latent_dim 384 / 512, and every later call failed)
    if (getenv("DSG_KSET")) {                  // an A/B run pinned the set for the whole process: say so once, keep the pinned set
        static std::atomic<bool> said{false};
        if (set != h->kset_req && !said.exchange(true))
            fprintf(stderr, "libdsg_hip: WARNING: DSG_KSET=%s pins the kernel set of every handle; dsg_set_kernel_set(%d) ignored "
                            "(dsg_get_kernel_set reports the set in force)\n", getenv("DSG_KSET"), set);
        return 0;
    }
    h->kset_req = set;
    return 0;
}
// the set in force for the handle (what dsg_set_kernel_set / DSG_KSET / dsg_clone left): callers that change it for one call
// (sample.generate_clips_streams) restore it afterwards
extern "C" int dsg_get_kernel_set(dsg_handle* h, int* set) {
    if (!h || !set) return fail(DSG_E_INVALID, "null argument");
    *set = h->kset_req;
    return 0;
}
extern "C" int dsg_recommend_kernel_set(dsg_handle* h, int B, int lanes, int* set) {
    if (!h || !set || B <= 0 || lanes <= 0) return fail(DSG_E_INVALID, "dsg_recommend_kernel_set: bad argument");
    *set = resolve_auto_set(h, B, lanes);
    return 0;
}
extern "C" int dsg_last_kernel_set(dsg_handle* h, int* set) {
    if (!h || !set) return fail(DSG_E_INVALID, "null argument");
    if (h->last.kset < 0) return fail(DSG_E_STATE, "no step has run");
    *set = h->last.kset;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// one denoising step = the pose embedding + local attention (k_in + k_loc; LATENCY: k_inloc), L layers of one form (2 .. 5 dispatches each,
// enum Form) and the pose head: 3 + 2L (ROWS / STREAM) .. 3 + 5L (TILE without k_attn_op), LATENCY 2 + 3L at batch 1
// ---------------------------------------------------------------------------------------------------------
struct StepCtx {
    int B;                  // batch rows the kernels run on (with guidance: conditional elements + their twins)
    int out_mode; bool use_ctr; const float* ext_noise; int const_noise;
    int keyed = 0;          // per-element noise streams (dsg_set_noise_streams)
    int no_noise = 0;       // DDIM with eta = 0: no step adds noise (the pose head skips the Philox draw)
    int clip_x0 = 0;        // clip_denoised=True
    int inpaint = 0;        // the handle's inpainting constraint applies (sampling only: MDM.forward does not inpaint)
    KernelSel ks;           // what select_kernels chose for this call
};

// Every kernel of the denoising step goes through here: a HIP launch on the handle's stream, or -- while dsg_sample is
// recording the step for the AQL path -- an entry of the packet plan (dsg_aql.h).
template <auto K, class A>
static int step_launch(dsg_handle* h, dim3 grid, dim3 block, const A& args) {
#ifndef DSG_EMU
    if (h->aql.recording) {
        const int fence = h->state_fences ? h->fence_next : 0;
        h->fence_next = 0;
        if (!dsg_aql::record(h->aql, (const void*)K, h->stream, grid, block, &args, sizeof(A), fence))
            return fail(DSG_E_RUNTIME, "AQL plan: " + h->aql.err);
        return 0;
    }
#endif
    h->fence_next = 0;
    hipLaunchKernelGGL(K, grid, block, 0, h->stream, args);
    HIPCHK(hipGetLastError());
    return 0;
}

// k-blocks per fragment batch of gemm_body (CH) for a wave whose k range is `per_wave` k-blocks: the fewest batches, then the
// fewest clamped (wasted) loads
static int pick_ch(int per_wave) {
    if (per_wave <= 8) return 8;
    if (per_wave <= 12) return 12;
    if (per_wave <= 16) return 16;
    if (per_wave % 16 == 0) return 16;
    if (per_wave % 12 == 0) return 12;
    return 8;
}
template <class P, int PRO, int EPI, int WN, int WK>
static int launch_gemm(dsg_handle* h, GemmArgs g) {
    if (g.KS == 1) g.kb_per_split = g.KBtot;
    const int NG = g.NT / WN;
    if (NG * WN != g.NT) return fail(DSG_E_INVALID, "gemm: NT not divisible by the workgroup tile");
    if (WK > 1 && (g.KS != 1 || g.KBtot % WK)) return fail(DSG_E_INVALID, "gemm: k-blocks not divisible by the wave split");
    if (g.KS < 1 || g.kb_per_split * g.KS < g.KBtot) return fail(DSG_E_INVALID, "gemm: split-K does not cover K");
    // EPI_PARTIAL / EPI_OUT carry one extra grid row whose first workgroup does the step bookkeeping
    const int extra = (EPI == EPI_PARTIAL || EPI == EPI_OUT) ? 1 : 0;
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    const dim3 grid(xcd_grid_x(NG), g.MT + extra, g.KS);
    // one batch of fragment loads per wave wherever the wave's k range allows it (gemm_body: CH)
    if constexpr (EPI != EPI_PARTIAL) {
        const int ch = pick_ch(std::min(g.kb_per_split, g.KBtot) / WK);
        if (ch == 16) return step_launch<&k_gemm<P, PRO, EPI, WN, WK, 1, 16>>(h, grid, dim3(256), g);
        if (ch == 12) return step_launch<&k_gemm<P, PRO, EPI, WN, WK, 1, 12>>(h, grid, dim3(256), g);
    }
    return step_launch<&k_gemm<P, PRO, EPI, WN, WK, 1>>(h, grid, dim3(256), g);
}
// 32-row x 64-column blocks, K = D whole (dsg_batched.h).  Measured per GEMM in the real batch-16 step
// (profiles/r02_c_blk_sweep.log): QKV -13 us, linear1 -7, embedding -9.5 per step; out_proj +4 and the pose head +3.5 (few,
// long workgroups) stay on the 16 x 16 kernels.  Wider / taller blocks (128-column waves, 64 rows) lose (335 -> 380 / 364 us).
template <class P, int PRO, int EPI>
static int launch_blk(dsg_handle* h, GemmArgs g) {
    g.KS = 1; g.kb_per_split = g.KBtot;
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    const int K = g.KBtot * P::KB;
    if (g.NT % 4) return fail(DSG_E_INVALID, "gemm: NT not divisible by the workgroup tile");
    const dim3 grid(xcd_grid_x(g.NT / 4), cdiv(g.MT, 2) + (EPI == EPI_OUT ? 1 : 0), 1);
    if (K <= 256) return step_launch<&k_gemm_blk<P, PRO, EPI, 256, 1, 2>>(h, grid, dim3(256), g);
    if (K > 512) return fail(DSG_E_NOT_IMPLEMENTED, "k_gemm_blk: K > 512");
    return step_launch<&k_gemm_blk<P, PRO, EPI, 512, 1, 2>>(h, grid, dim3(256), g);
}
template <class P, int EPI>
static int launch_blk_k(dsg_handle* h, GemmArgs g) {
    if (g.KS <= 1) { g.KS = 1; g.kb_per_split = g.KBtot; }
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    if (g.NT % 2) return fail(DSG_E_INVALID, "gemm: NT not divisible by the workgroup tile");
    const int extra = EPI == EPI_PARTIAL ? 1 : 0;
    const dim3 grid(xcd_grid_x(g.NT / 2), cdiv(g.MT, 2) + extra, g.KS);
    // k-blocks per wave in one pass: 8 when the wave's share of the K range is that long (linear2 at ff = 1024 in bf16), else 4
    const int per = cdiv(std::min(g.kb_per_split, g.KBtot), 4);
    if (per > 4) return step_launch<&k_gemm_blk_k<P, EPI, 8>>(h, grid, dim3(256), g);
    return step_launch<&k_gemm_blk_k<P, EPI, 4>>(h, grid, dim3(256), g);
}

// STREAM (dsg_stream.h): persistent grid = 128-column panels x row-block groups.  Groups: enough workgroups for `occ` per CU,
// never more than there are row blocks, a multiple of 8 (one group per XCD slot)
static int ws_groups(int n_panels, int n_blocks, int occ) {
    int G = (256 * occ / n_panels) & ~7;
    G = std::max(G, 8);
    return std::min(G, rup(n_blocks, 8));
}
template <int EPI>
static int launch_ws(dsg_handle* h, GemmArgs g) {
    g.KS = 1; g.kb_per_split = g.KBtot;
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    if (g.NT % 8) return fail(DSG_E_INVALID, "k_ws: N must be a multiple of 128");
    const int P = g.NT / 8, MB = cdiv(g.M, 64);
    g.ws_G = ws_groups(P, MB, 2);
    const int K = g.KBtot * 32;
    if constexpr (EPI == EPI_OUT) {
        // the pose head: one workgroup per (panel, row block), three per CU (round 5; the persistent row-block groups of rounds 3-4 lost on two
        // boxes and are retired -- experiments/README.md) + the bookkeeping workgroup (one XCD round)
        g.ws_G = rup(MB, 8);
        const dim3 grid1(ws_grid_x(P, g.ws_G) + 8);
        if (K == 256) return step_launch<&k_ws<EPI, 16, true>>(h, grid1, dim3(256), g);
        if (K == 128) return step_launch<&k_ws<EPI, 8, true>>(h, grid1, dim3(256), g);
        if (K == 384) return step_launch<&k_ws<EPI, 24, true>>(h, grid1, dim3(256), g);      // (round 6: the DSG+ widths, one workgroup per CU)
        if (K == 512) return step_launch<&k_ws<EPI, 32, true>>(h, grid1, dim3(256), g);
    } else {
        const dim3 grid(ws_grid_x(P, g.ws_G));
        if (K == 256) return step_launch<&k_ws<EPI, 16>>(h, grid, dim3(256), g);
        if (K == 128) return step_launch<&k_ws<EPI, 8>>(h, grid, dim3(256), g);
    }
    return fail(DSG_E_NOT_IMPLEMENTED, "k_ws: K must be 128 or 256");
}
// the guided streaming pose head (k_ws_cfg): one workgroup per (panel, block of 32 conditional rows) + the bookkeeping workgroup; g.M / g.B: the conditional half
static int launch_ws_cfg(dsg_handle* h, GemmArgs g) {
    g.KS = 1; g.kb_per_split = g.KBtot;
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    if (g.NT % 8) return fail(DSG_E_INVALID, "k_ws_cfg: N must be a multiple of 128");
    const int P = g.NT / 8, K = g.KBtot * 32;
    g.ws_G = rup(cdiv(g.M, 32), 8);
    const dim3 grid(ws_grid_x(P, g.ws_G) + 8);
    if (K == 384) return step_launch<&k_ws_cfg<24>>(h, grid, dim3(256), g);
    if (K == 512) return step_launch<&k_ws_cfg<32>>(h, grid, dim3(256), g);
    return fail(DSG_E_NOT_IMPLEMENTED, "k_ws_cfg: K must be 384 or 512");
}
// STREAM: LayerNorm once per row (k_ln_frag) -> fragment-major bf16 rows in X1a (free between linear1 and the next attention
// kernel) [+ fp32 rows in Xn], then the GEMM streams them like linear1.  Packet fences of the state (fence_next) belong to the GEMM.
template <int EPI>
static int launch_ln_ws(dsg_handle* h, GemmArgs g) {
    const int fence = h->fence_next;
    h->fence_next = 0;
    GemmArgs l = g;
    l.out = h->X1a;
    const dim3 grid(cdiv(rup(g.M, 64), 16));
    switch (h->core) {
        case Core::C256: CHK((step_launch<&k_ln_frag<4>>(h, grid, dim3(256), l))); break;
        case Core::C128: CHK((step_launch<&k_ln_frag<2>>(h, grid, dim3(256), l))); break;
        default: return fail(DSG_E_NOT_IMPLEMENTED, "k_ln_frag: latent_dim must be 128 or 256");
    }
    h->fence_next = fence;
    g.A = h->X1a; g.lda = g.D; g.a_frag = 1; g.X = nullptr; g.Xn = nullptr;
    return launch_ws<EPI>(h, g);
}
template <int EPI>
static int launch_ws2(dsg_handle* h, GemmArgs g) {
    g.KS = 1; g.kb_per_split = g.KBtot;
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    if (g.NT % 4) return fail(DSG_E_INVALID, "k_ws2: N must be a multiple of 64");
    const int K = g.KBtot * 32;
    const int ksplit = (EPI == EPI_PARTIAL && K > 1152) ? 2 : 1;      // (the DSG+ pose widths: K over two workgroups, two slabs for k_loc -- see k_ws2)
    const int P = g.NT / 4 * ksplit, MB = cdiv(g.M, 32);
    g.ws_G = ws_groups(P, MB, 1);
    g.KS = ksplit;
    const dim3 grid(ws_grid_x(P, g.ws_G) + (EPI == EPI_PARTIAL ? 8 : 0));      // EPI_PARTIAL: + the bookkeeping workgroup
    if constexpr (EPI == EPI_RESID) {
        if (K == 1024) return step_launch<&k_ws2<EPI, 16>>(h, grid, dim3(256), g);
        if (K == 128) return step_launch<&k_ws2<EPI, 2>>(h, grid, dim3(256), g);
    } else {
        if (K == 1152) return step_launch<&k_ws2<EPI, 18>>(h, grid, dim3(256), g);
        if (K == 128) return step_launch<&k_ws2<EPI, 2>>(h, grid, dim3(256), g);
        if (K == 2176) return step_launch<&k_ws2<EPI, 17, 2>>(h, grid, dim3(256), g);      // BEAT (round 6)
        if (K == 2304) return step_launch<&k_ws2<EPI, 18, 2>>(h, grid, dim3(256), g);      // TWH
    }
    return fail(DSG_E_NOT_IMPLEMENTED, "k_ws2: K must be 128 / 1024 (linear2) or 128 / 1152 / 2176 / 2304 (pose embedding)");
}

// a K = D GEMM of the un-fused sets: block kernel (BLOCK, the GEMMs it wins), else 16 x 16 tiles -- LayerNorm GEMMs from 512
// rows in the 3-waves-per-SIMD form (k_gemm_lean; tools/b16_lean.sh: batch 8: 250 vs 267 us/step, batch 16: 360 vs 378)
template <class P, int PRO, int EPI>
static int launch_gemm_w(dsg_handle* h, const GemmArgs& g, const KernelSel& ks) {
    constexpr bool blk_wins = EPI == EPI_QKV || EPI == EPI_GELU;
    if constexpr (sizeof(typename P::elem) == 2 && !P::W2 && PRO == PRO_DIRECT && (EPI == EPI_GELU || EPI == EPI_QKV || EPI == EPI_OUT)) {
        if (ks.stream() && g.a_frag) return launch_ws<EPI>(h, g);      // STREAM: linear1 on the fragment-major LayerNorm1 rows of k_attn_op
        // (the streaming pose head below the STREAM sizes loses: BLOCK 1 x 16 clips 207.5 -> 211.6 us per step, 4 x 4: 197.5 -> 205.4 -- profiles/r06_h_*, round 6)
        // (... at the DSG+ widths it wins or is even everywhere in ROWS -- k_ws<OUT, 24 / 32, ONE>: 112 VGPRs + 32 AGPRs, the panel re-read per block: BEAT 1 x 16 clips
        //  358.3 -> 353.8 us per step, 4 x 8: 440.9 -> 423.3, 4 x 16: 615.6 -> 568.3; TWH 1 x 16 even, 4 x 16: 878 -> 844 -- profiles/r06_ds_*; 32 x 32 x 16 MFMAs: the
        //  pose head's last bits differ from the 16 x 16 tiles', so it belongs to the set, not to the lane count)
        if constexpr (EPI == EPI_OUT) {
            if (ks.form == Form::CLIP_W_FFN && g.a_frag) return launch_ws<EPI>(h, g);
        }
    }
    if constexpr (sizeof(typename P::elem) == 2 && !P::W2 && PRO == PRO_LN && (EPI == EPI_QKV || EPI == EPI_OUT)) {
        if (ks.stream()) return launch_ln_ws<EPI>(h, g);                    // STREAM: LayerNorm once per row, then the same streaming GEMM
    }
    if constexpr (EPI != EPI_PARTIAL && !P::W2) {
        if (ks.blk() && blk_wins && g.KBtot * P::KB <= 512) return launch_blk<P, PRO, EPI>(h, g);
    }
    if constexpr (PRO == PRO_LN) {
        if (g.M >= 512) {
            GemmArgs gl = g;
            gl.KS = 1; gl.kb_per_split = gl.KBtot;
            gl.inv_ntok = fastdiv_inv(gl.ntok); gl.inv_hd = fastdiv_inv(gl.hd);
            if (gl.NT % 4) return fail(DSG_E_INVALID, "gemm: NT not divisible by the workgroup tile");
            const dim3 grid(xcd_grid_x(gl.NT / 4), gl.MT + (EPI == EPI_OUT ? 1 : 0), 1);
            if constexpr (!P::W2) {      // (bf16w2: 16 k-blocks of two-register weight + activation fragments do not fit: two batches of 8)
                if (pick_ch(gl.KBtot) == 16) return step_launch<&k_gemm_lean<P, EPI, 16>>(h, grid, dim3(256), gl);
            }
            if (pick_ch(gl.KBtot) == 12) return step_launch<&k_gemm_lean<P, EPI, 12>>(h, grid, dim3(256), gl);
            return step_launch<&k_gemm_lean<P, EPI>>(h, grid, dim3(256), gl);
        }
    }
    return launch_gemm<P, PRO, EPI, 4, 1>(h, g);
}
// linear2: K = ff split over the 4 waves of the workgroup
template <class P>
static int launch_gemm_k4(dsg_handle* h, const GemmArgs& g, const KernelSel& ks) {
    if constexpr (sizeof(typename P::elem) == 2 && !P::W2) {
        if (ks.stream() && g.a_frag) return launch_ws2<EPI_RESID>(h, g);
    }
    if constexpr (!P::W2) {
        if (ks.blk()) return launch_blk_k<P, EPI_RESID>(h, g);
    }
    return launch_gemm<P, PRO_DIRECT, EPI_RESID, 1, 4>(h, g);
}

template <class P, int HD, int NKT>
static int launch_attn_t(dsg_handle* h, const AttnArgs& a) {
    const int nqt = cdiv(a.ntok, 16);
    return step_launch<&k_attn<P, HD, NKT>>(h, dim3(nqt, a.H, a.B), dim3(64), a);
}
template <class P>
static int launch_attn(dsg_handle* h, int B) {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = h->q; a.k = h->k; a.vt = h->vt; a.out = h->attn; a.B = B; a.H = h->H; a.ntok = h->ntok; a.Tp = h->Tp; a.D = h->D;
    const int key = h->hd * 1000 + h->Tp / 16;
    switch (key) {
        case 32 * 1000 + 2: return launch_attn_t<P, 32, 2>(h, a);
        case 64 * 1000 + 2: return launch_attn_t<P, 64, 2>(h, a);
        case 64 * 1000 + 6: return launch_attn_t<P, 64, 6>(h, a);
        case 96 * 1000 + 10: return launch_attn_t<P, 96, 10>(h, a);
        case 128 * 1000 + 10: return launch_attn_t<P, 128, 10>(h, a);
        default: return fail(DSG_E_NOT_IMPLEMENTED, "no attention instantiation for (head_dim, tokens) = (" +
                                                        std::to_string(h->hd) + ", " + std::to_string(h->Tp) + ")");
    }
}

// k_loc / k_inloc are instantiated per (local head dim, window).  INLOC: k_inloc (LATENCY), else k_loc with NT threads per (head, window, clip):
// 256, or 128 = its two-wave form (round 6: see the call site)
template <class P, bool INLOC, int NT, int HD, int W, class A>
static int launch_loc_t(dsg_handle* h, dim3 grid, const A& a) {
    if constexpr (INLOC) return step_launch<&k_inloc<P, HD, W>>(h, grid, dim3(NT), a);
    else return step_launch<&k_loc<P, HD, W, NT>>(h, grid, dim3(NT), a);
}
template <class P, bool INLOC, int NT, class A>
static int launch_loc(dsg_handle* h, dim3 grid, const A& a) {
    switch (h->hdl * 100 + h->W) {
        case 32 * 100 + 11: return launch_loc_t<P, INLOC, NT, 32, 11>(h, grid, a);
        case 48 * 100 + 15: return launch_loc_t<P, INLOC, NT, 48, 15>(h, grid, a);
        case 64 * 100 + 15: return launch_loc_t<P, INLOC, NT, 64, 15>(h, grid, a);
        case 16 * 100 + 11: return launch_loc_t<P, INLOC, NT, 16, 11>(h, grid, a);
        case 8 * 100 + 15: return launch_loc_t<P, INLOC, NT, 8, 15>(h, grid, a);
        default: return fail(DSG_E_NOT_IMPLEMENTED, "no local-attention instantiation for (head dim, window) = (" +
                                                        std::to_string(h->hdl) + ", " + std::to_string(h->W) + ")");
    }
}

template <class P>
static int launch_mid(dsg_handle* h, const MidArgs& a) {
    const dim3 grid(xcd_grid_x(a.ff / 64), a.MT);
    switch (h->D / 64) {      // (any head count: k_mid is instantiated per latent_dim, not per core)
        case 1: return step_launch<&k_mid<P, 1>>(h, grid, dim3(256), a);
        case 2: return step_launch<&k_mid<P, 2>>(h, grid, dim3(256), a);
        case 4: return step_launch<&k_mid<P, 4>>(h, grid, dim3(256), a);
        // (bf16w2: two-register weight fragments, LATENCY up to latent_dim 256 -- check_set)
        case 6: if constexpr (!P::W2) return step_launch<&k_mid<P, 6>>(h, grid, dim3(256), a); break;
        case 8: if constexpr (!P::W2) return step_launch<&k_mid<P, 8>>(h, grid, dim3(256), a); break;
        default: break;
    }
    return fail(DSG_E_NOT_IMPLEMENTED, "k_mid: latent_dim / 64 must be 1, 2, 4, 6 or 8 (bf16w2: 1, 2 or 4)");
}
// Attention fused into k_mid: one batch element, 4 heads (wave = head), D <= 256.  Bit-identical to k_attn + k_mid and
// one dispatch less per layer.  With HIP launches it does not pay (152.4 vs 151.3 us/step): the four heads' strided
// K / V^T fragment loads queue on ONE CU's load path (38 loads in ~6100 cycles) instead of running on 24 otherwise idle
// CUs, which costs what the saved launch gains.  With the AQL submission the balance tips (136.0 vs 140.8 us/step,
// measured twice on the same box), so it is what batch 1 runs (batch 2 of the same set runs k_attn + k_mid: tests compare the two).
template <class P>
static int launch_attn_mid(dsg_handle* h, const AttnMidArgs& a) {
    const dim3 grid(xcd_grid_x(a.mid.ff / 64), a.mid.MT);
    switch (h->core) {
        case Core::C256: return step_launch<&k_attn_mid<P, 4, 6>>(h, grid, dim3(256), a);
        case Core::C128: return step_launch<&k_attn_mid<P, 2, 2>>(h, grid, dim3(256), a);
        default: return fail(DSG_E_NOT_IMPLEMENTED, "no fused attention+mid instantiation");
    }
}

static StepTables step_tables(const dsg_handle* h) {
    StepTables st;
    st.tmodel = h->st_tmodel; st.c1 = h->st_c[0]; st.c2 = h->st_c[1]; st.c3 = h->st_c[2]; st.c4 = h->st_c[3]; st.c5 = h->st_c[4];
    return st;
}

// the GemmArgs every GEMM of a step of B batch rows starts from
static GemmArgs gemm_base(const dsg_handle* h, int B) {
    GemmArgs z;
    memset(&z, 0, sizeof(z));
    z.KS = 1; z.B = B; z.ntok = h->ntok; z.Tp = h->Tp; z.H = h->H; z.hd = h->hd; z.T = h->T; z.J = h->J; z.Jp = h->Jp;
    z.Jq = h->Jq; z.D = h->D; z.inv_ntok4 = fastdiv_inv(rup(h->ntok, 4));
    return z;
}
// One builder per GEMM of the step (the layer functions, run_step and debug_launch start from these).  M = the rows it runs on.
static GemmArgs gemm_of(const dsg_handle* h, const GemmArgs& z, int M, int N, int K, const void* Wp, const float* bias) {
    GemmArgs g = z;
    g.M = M; g.MT = cdiv(M, 16); g.NT = N / 16; g.KBtot = K / h->kbk; g.Wp = Wp; g.bias = bias;
    return g;
}
// k_in: partial[s] = xs[:, chunk s] . Wfold[:, chunk s]^T over KS workgroup splits of K (the step adds its control block: step_ctl)
static GemmArgs gemm_pose_in(const dsg_handle* h, const GemmArgs& z, int Min, int KS) {
    GemmArgs g = gemm_of(h, z, Min, h->D, h->Jp, h->Wp_in, nullptr);
    g.KS = KS; g.kb_per_split = cdiv(g.KBtot, g.KS);
    g.A = is_bf16(h) ? h->xsA : (void*)h->xs32; g.lda = h->Jp; g.out = h->partial; g.ldo = h->D;
    return g;
}
// QKV -> q / k / v^T: on the rows in X0a (in_frag >= 0: their layout) or on pre2 with LayerNorm2 of layer `prev` applied on read (-> Xn)
static GemmArgs gemm_qkv(const dsg_handle* h, const GemmArgs& z, int M, const Layer& ly, int in_frag, const Layer* prev) {
    GemmArgs g = gemm_of(h, z, M, 3 * h->D, h->D, ly.Wqkv, ly.bqkv);
    g.q = h->q; g.k = h->k; g.vt = h->vt;
    if (in_frag >= 0) { g.A = h->X0a; g.lda = h->D; g.a_frag = in_frag; }
    else { g.X = h->pre2; g.ln_g = prev->g2; g.ln_b = prev->be2; g.Xn = h->Xn; }
    return g;
}
static GemmArgs gemm_out_proj(const dsg_handle* h, const GemmArgs& z, int M, const Layer& ly, const float* R) {      // + residual R -> pre1
    GemmArgs g = gemm_of(h, z, M, h->D, h->D, ly.Wo, ly.bo);
    g.A = h->attn; g.lda = h->D; g.a_frag = 1; g.out = h->pre1; g.ldo = h->D; g.R = R;
    return g;
}
// linear1 + GELU -> hidden: with LayerNorm1 of pre1 on read (X1 = LN1(pre1)), or (frag) on k_attn_op's fragment-major LayerNorm1 rows
static GemmArgs gemm_linear1(const dsg_handle* h, const GemmArgs& z, int M, const Layer& ly, bool frag) {
    GemmArgs g = gemm_of(h, z, M, h->ff, h->D, ly.W1, ly.b1);
    if (frag) { g.A = h->X1a; g.lda = h->D; g.a_frag = 1; }
    else { g.X = h->pre1; g.ln_g = ly.g1; g.ln_b = ly.be1; g.Xn = h->X1; }
    g.out = h->hidden; g.ldo = h->ff; g.out_frag = 1;
    return g;
}
static GemmArgs gemm_linear2(const dsg_handle* h, const GemmArgs& z, int M, const Layer& ly) {      // + residual X1 -> pre2
    GemmArgs g = gemm_of(h, z, M, h->D, h->ff, ly.W2, ly.b2);
    g.A = h->hidden; g.lda = h->ff; g.a_frag = 1; g.out = h->pre2; g.ldo = h->D; g.R = h->X1;
    return g;
}
// pose head on pre2 with LayerNorm2 of layer `last` on read + the sampler update (the step adds out_mode, noise and its control block)
static GemmArgs gemm_pose_head(const dsg_handle* h, const GemmArgs& z, int M, const Layer& last) {
    GemmArgs g = gemm_of(h, z, M, h->Jp, h->D, h->Wp_out, h->b_out);
    g.X = h->pre2; g.ln_g = last.g2; g.ln_b = last.be2;
    g.xs32 = h->xs32; g.xsA = is_bf16(h) ? h->xsA : nullptr; g.fwd_out = h->fwd_out; g.dyn = h->dyn; g.draw_off = h->dyn + GemmArgs::dyn_pairs(h->Bmax);
    return g;
}
// the step control of the two GEMMs that read / advance it (k_in, pose head)
static void step_ctl(const dsg_handle* h, GemmArgs& g, StepCtl* ctl) { g.ctl = ctl; g.st = step_tables(h); g.n_tab = h->n_run; }
// k_loc / k_inloc: the embedding's KS partial sums -> the local attention -> X0 (fp32) + X0a (in the layout x0a_frag)
static LocArgs loc_args(const dsg_handle* h, int B, int KS, const StepCtl* ctl, int x0a_frag) {
    LocArgs la;
    memset(&la, 0, sizeof(la));
    la.partial = h->partial; la.KS = KS; la.Min_pad = cdiv(B * h->T, 16) * 16; la.Cf = h->Cf; la.TE2 = h->TE2; la.TE = h->TE;
    la.emb1 = h->emb1; la.ctl = ctl; la.t_arr = h->t_arr;
    la.rcos = h->rcos; la.rsin = h->rsin; la.mask = h->mask; la.mb = h->mb; la.inv_mask_div = fastdiv_inv((int)((long long)B * h->Hl / h->mb)); la.B = B; la.T = h->T; la.D = h->D; la.Hl = h->Hl;
    la.hd = h->hdl; la.W = h->W; la.X0 = h->X0; la.X0a = h->X0a; la.nomask = h->nomask; la.x0a_frag = x0a_frag;
    return la;
}
static InLocArgs inloc_args(const dsg_handle* h, const LocArgs& la, StepCtl* ctl_upd, int n_tab) {
    InLocArgs a;
    a.xs = is_bf16(h) ? h->xsA : (void*)h->xs32; a.Jp = h->Jp; a.Wp = h->Wp_in; a.KBtot = h->Jp / h->kbk;
    a.loc = la; a.ctl_upd = ctl_upd; a.st = step_tables(h); a.n_tab = n_tab;
    return a;
}
static MidArgs mid_args(const dsg_handle* h, const Layer& ly, const float* R, int M) {
    MidArgs a;
    memset(&a, 0, sizeof(a));
    a.A = h->attn; a.R = R; a.Wo = ly.Wo; a.bo = ly.bo; a.ln_g = ly.g1; a.ln_b = ly.be1;
    a.W1 = ly.W1; a.b1 = ly.b1; a.X1 = h->X1; a.hidden = h->hidden; a.M = M; a.MT = cdiv(M, 16); a.ff = h->ff;
    return a;
}

// What one encoder layer's launches read
struct LayerCtx {
    const KernelSel& ks;
    const GemmArgs& z;      // gemm_base of the step
    const Layer& ly;
    int M, MT;
    const float* R;         // the rows the attention block adds back: the embedding (X0) in layer 0, LayerNorm2 of the previous layer (Xn) after it
    int in_frag;            // where the layer's input rows are: X0a in that layout (layer 0: ks.x0a_frag; after a form that leaves X0a: 1), or
    const Layer* prev;      // -1: pre2, with LayerNorm2 of the previous layer (prev) applied on read
};
static ClipAttnArgs clip_attn_args(const dsg_handle* h, const LayerCtx& y) {
    ClipAttnArgs a;
    a.X = h->X0a; a.Wqkv = y.ly.Wqkv; a.bqkv = y.ly.bqkv; a.out = h->attn; a.B = y.z.B; a.ntok = h->ntok;
    return a;
}
// k_ffn: linear1 + GELU + linear2 + residual + LayerNorm2 -> Xn fp32 + X0a in the GEMM type.  OP: out_proj + residual + LayerNorm1
// as the prologue (A = the attention rows); else A = k_attn_op's fragment-major LayerNorm1 rows
static FfnArgs ffn_args(const dsg_handle* h, const LayerCtx& y, bool op) {
    const Layer& ly = y.ly;
    FfnArgs a;
    memset(&a, 0, sizeof(a));
    a.A = h->X1a; a.R = h->X1; a.W1 = ly.W1; a.b1 = ly.b1; a.W2 = ly.W2; a.b2 = ly.b2; a.ln_g = ly.g2; a.ln_b = ly.be2;
    a.Xn = h->Xn; a.Xa = h->X0a; a.M = y.M; a.MT = y.MT;
    if (op) { a.A = h->attn; a.R = y.R; a.Wo = ly.Wo; a.bo = ly.bo; a.ln1_g = ly.g1; a.ln1_b = ly.be1; a.X1 = h->X1; }
    return a;
}

// ---- the launches the layer forms share
template <class P>
static int qkv_gemm(dsg_handle* h, const LayerCtx& y) {
    const GemmArgs g = gemm_qkv(h, y.z, y.M, y.ly, y.in_frag, y.prev);
    if (y.in_frag >= 0) return launch_gemm_w<P, PRO_DIRECT, EPI_QKV>(h, g, y.ks);
    return launch_gemm_w<P, PRO_LN, EPI_QKV>(h, g, y.ks);
}
// attention + out_proj + residual + LayerNorm1 in one kernel per (query tile, batch element); the next kernel reads the normalised rows in the
// GEMM type (k_attn_op2 -- two query tiles per workgroup -- is retired: experiments/dsg_rejected_kernels.h)
template <class P>
static int attn_op(dsg_handle* h, const LayerCtx& y) {
    const Layer& ly = y.ly;
    AttnOpArgs a;
    a.q = h->q; a.k = h->k; a.vt = h->vt; a.R = y.R; a.Wo = ly.Wo; a.bo = ly.bo; a.ln_g = ly.g1; a.ln_b = ly.be1;
    a.X1 = h->X1; a.X1a = h->X1a; a.B = y.z.B; a.ntok = h->ntok; a.Tp = h->Tp;
    const dim3 grid(cdiv(h->ntok, 16), y.z.B);
    if constexpr (sizeof(typename P::elem) == 2) {
        switch (h->core) {
            case Core::C256: return step_launch<&k_attn_op<P, 4, 6>>(h, grid, dim3(256), a);
            case Core::C128: return step_launch<&k_attn_op<P, 2, 2>>(h, grid, dim3(256), a);
            case Core::C384: return step_launch<&k_attn_op_w<P, 6, 10>>(h, grid, dim3(256), a);
            case Core::C512: return step_launch<&k_attn_op_w<P, 8, 10>>(h, grid, dim3(256), a);
            default: break;
        }
    } else {
        switch (h->core) {
            case Core::C256: return step_launch<&k_attn_op_w<P, 4, 6>>(h, grid, dim3(256), a);
            case Core::C128: return step_launch<&k_attn_op_w<P, 2, 2>>(h, grid, dim3(256), a);
            default: break;
        }
    }
    return no_inst(h, "k_attn_op");
}
// round 5: per (clip, head) -- QKV slices + attention in one kernel (k_clip_attn); out_proj + residual + LayerNorm1 are the prologue of the
// feed-forward kernel behind it (OP): Q / K / V never leave the CU and the QKV GEMM is gone as a dispatch
template <class P>
static int clip_attn(dsg_handle* h, const LayerCtx& y) {
    const ClipAttnArgs a = clip_attn_args(h, y);
    switch (h->core) {
        case Core::C256: return step_launch<&k_clip_attn<P, 4, 6>>(h, dim3(4, y.z.B), dim3(384), a);
        case Core::C128: return step_launch<&k_clip_attn<P, 2, 2>>(h, dim3(4, y.z.B), dim3(128), a);
        default: return no_inst(h, "k_clip_attn");
    }
}
template <class P>
static int linear2(dsg_handle* h, const LayerCtx& y) { return launch_gemm_k4<P>(h, gemm_linear2(h, y.z, y.M, y.ly), y.ks); }      // (K = ff split over the 4 waves of the workgroup)
// BLOCK below the STREAM threshold (round 4): k_ffn split over the hidden dimension (k_ffn_part) + the slab sum / LayerNorm2 pass (k_ffn_ln).
// profiles/r04_q_*: 1 x 16 230.9 -> 218.8 us, 4 x 4 222.4 -> 214.4, 4 x 8 288.9 -> 240.8.  OP: out_proj + residual + LayerNorm1 as the prologue
template <class P, int DT, int FT, int S, bool OP>      // latent_dim = 64 DT, ff = 64 FT, S ff-splits (= slabs)
static int ffn_split_t(dsg_handle* h, const LayerCtx& y, const FfnPartArgs& a, const FfnLnArgs& b) {
    CHK((step_launch<&k_ffn_part<P, DT, FT, 2, 4, S, OP>>(h, dim3(cdiv(y.MT, 2) * S), dim3(256), a)));
    return step_launch<&k_ffn_ln<P, DT, S, 8>>(h, dim3(cdiv(y.M, 8)), dim3(128), b);
}
template <class P, bool OP>
static int ffn_split(dsg_handle* h, const LayerCtx& y) {
    const Layer& ly = y.ly;
    FfnPartArgs a;
    memset(&a, 0, sizeof(a));
    a.A = h->X1a; a.W1 = ly.W1; a.b1 = ly.b1; a.W2 = ly.W2; a.part = h->ffn_part; a.slab = h->ffn_slab; a.M = y.M; a.MT = y.MT;
    if (OP) { a.A = h->attn; a.R = y.R; a.Wo = ly.Wo; a.bo = ly.bo; a.ln_g = ly.g1; a.ln_b = ly.be1; a.X1 = h->X1; }
    FfnLnArgs b;
    b.part = h->ffn_part; b.slab = h->ffn_slab; b.R = h->X1; b.b2 = ly.b2; b.ln_g = ly.g2; b.ln_b = ly.be2; b.Xn = h->Xn; b.Xa = h->X0a; b.M = y.M;
    if constexpr (sizeof(typename P::elem) == 4) {
        // fp32 at the ZEGGS widths (round 5, round-4 verdict item 7): the same split, 8 ways (16 k-blocks of 16 per K = 256 operand)
        if (h->core == Core::C256) return ffn_split_t<P, 4, 16, 8, false>(h, y, a, b);
    } else {
        switch (h->core) {
            case Core::C256: return ffn_split_t<P, 4, 16, 4, OP>(h, y, a, b);
            case Core::C128: return ffn_split_t<P, 2, 2, 2, OP>(h, y, a, b);
            // DSG+ widths (round 5, k_attn_op_w only): 8 ff-splits, one row tile per workgroup-pair batch of fragments
            case Core::C384: return ffn_split_t<P, 6, 16, 8, false>(h, y, a, b);
            case Core::C512: return ffn_split_t<P, 8, 16, 8, false>(h, y, a, b);
            default: break;
        }
    }
    return no_inst(h, "k_ffn_part");
}

// ---- one function per layer form (enum Form): the launches of one encoder layer, in order
template <class P>
static int layer_mid(dsg_handle* h, const LayerCtx& y) {
    CHK(qkv_gemm<P>(h, y));
    const MidArgs a = mid_args(h, y.ly, y.R, y.M);      // [attention +] out_proj + residual + LayerNorm1 + linear1 slice + GELU
    if (y.ks.attn_in_mid) {
        AttnMidArgs am;
        am.mid = a; am.q = h->q; am.k = h->k; am.vt = h->vt; am.ntok = h->ntok; am.Tp = h->Tp;
        CHK(launch_attn_mid<P>(h, am));
    } else {
        CHK(launch_attn<P>(h, y.z.B));
        CHK(launch_mid<P>(h, a));
    }
    return linear2<P>(h, y);
}
template <class P>
static int layer_unfused(dsg_handle* h, const LayerCtx& y) {
    CHK(qkv_gemm<P>(h, y));
    CHK(launch_attn<P>(h, y.z.B));
    CHK((launch_gemm_w<P, PRO_DIRECT, EPI_RESID>(h, gemm_out_proj(h, y.z, y.M, y.ly, y.R), y.ks)));
    CHK((launch_gemm_w<P, PRO_LN, EPI_GELU>(h, gemm_linear1(h, y.z, y.M, y.ly, false), y.ks)));
    return linear2<P>(h, y);
}
template <class P>
static int layer_attn_op(dsg_handle* h, const LayerCtx& y) {
    CHK(qkv_gemm<P>(h, y));
    CHK(attn_op<P>(h, y));
    CHK((launch_gemm_w<P, PRO_DIRECT, EPI_GELU>(h, gemm_linear1(h, y.z, y.M, y.ly, true), y.ks)));
    return linear2<P>(h, y);
}
template <class P>
static int layer_attn_op_split(dsg_handle* h, const LayerCtx& y) {
    CHK(qkv_gemm<P>(h, y));
    CHK(attn_op<P>(h, y));
    return ffn_split<P, false>(h, y);
}
template <class P>
static int layer_clip_split(dsg_handle* h, const LayerCtx& y) {
    CHK(clip_attn<P>(h, y));
    return ffn_split<P, true>(h, y);
}
// 64 rows per workgroup when several lanes fill the GPU with large batches: half the weight bytes through the CUs' load paths per row, half
// the workgroups (select_kernels)
template <class P>
static int layer_attn_op_ffn(dsg_handle* h, const LayerCtx& y) {
    CHK(qkv_gemm<P>(h, y));
    CHK(attn_op<P>(h, y));
    const FfnArgs f = ffn_args(h, y, false);
    switch (h->core) {
        case Core::C256:
            if (y.ks.ffn_rows == 64) return step_launch<&k_ffn<P, 4, 16, 4, 8, 1, true>>(h, dim3(cdiv(y.MT, 4)), dim3(512), f);
            return step_launch<&k_ffn<P, 4, 16, 2, 8, 2, true>>(h, dim3(cdiv(y.MT, 2)), dim3(512), f);
        case Core::C128: return step_launch<&k_ffn<P, 2, 2, 2, 4>>(h, dim3(cdiv(y.MT, 2)), dim3(256), f);      // (32-row blocks only: select_kernels, rt4)
        default: return no_inst(h, "k_ffn");
    }
}
// (the weights of both phases on one rolling ring of fragments: 12 slots on 64-row blocks, 32 on 16- / 32-row blocks; the double-buffered groups of
//  rounds 4-5 are retired)
template <class P>
static int layer_clip_ffn(dsg_handle* h, const LayerCtx& y) {
    CHK(clip_attn<P>(h, y));
    const FfnArgs f = ffn_args(h, y, true);
    const int MT = y.MT, rows = y.ks.ffn_rows;
    // ROWS: one 16-row tile per workgroup (bf16w2, round 6: the only form, two-register fragments on a shorter ring); STREAM: 32-row blocks, C256: 64 as well (rt4)
    constexpr int RING256 = P::W2 ? 12 : 32, RING128 = P::W2 ? 8 : 0;
    switch (h->core) {
        case Core::C256:
            if (P::W2 || rows == 16) return step_launch<&k_ffn<P, 4, 16, 1, 8, 2, true, true, RING256>>(h, dim3(MT), dim3(512), f);
            if constexpr (!P::W2) {
                if (rows == 64) return step_launch<&k_ffn<P, 4, 16, 4, 8, 1, true, true, 12>>(h, dim3(cdiv(MT, 4)), dim3(512), f);
                return step_launch<&k_ffn<P, 4, 16, 2, 8, 2, true, true, 32>>(h, dim3(cdiv(MT, 2)), dim3(512), f);
            }
            break;
        case Core::C128:
            if (P::W2 || rows == 16) return step_launch<&k_ffn<P, 2, 2, 1, 4, 2, false, true, RING128>>(h, dim3(MT), dim3(256), f);
            if constexpr (!P::W2) return step_launch<&k_ffn<P, 2, 2, 2, 4, 2, false, true>>(h, dim3(cdiv(MT, 2)), dim3(256), f);
            break;
        default: break;
    }
    return no_inst(h, "k_ffn<OP>");
}
// ROWS at the DSG+ widths (round 6): QKV slices + attention per (clip, head) -- k_clip_attn_w (dsg_stream.h) -- and k_ffn<OP>
template <class P>
static int layer_clip_w_ffn(dsg_handle* h, const LayerCtx& y) {
    const int B = y.z.B, MT = y.MT;
    const ClipAttnArgs a = clip_attn_args(h, y);
    // one pass over the rows at both widths -- 384: three column tiles on waves 0 - 1 (144 weight registers fit: 236 VGPRs; the two-pass form: 1 x 16 clips
    // 371.3 vs 360.0 us per step, 4 x 16: 614 vs 604 -- profiles/r06_dq_*); 512: 192 weight registers, so the bias waits in the LDS and the A fragments have no
    // look-ahead (254 VGPRs).  The two-pass form (Q / K, then V in pairs on waves 0 - 3) read the rows from the LDS 1.5 times and reloaded weights in between:
    // TWH 1 x 16 clips 475.1 vs 472.9 us per step, 4 x 8: 601 vs 585, 4 x 16: 836.7 vs 830.1, bit-identical -- profiles/r06_dw_*; since retired
    switch (h->core) {
        case Core::C384: CHK((step_launch<&k_clip_attn_w<6, 10, 4>>(h, dim3(4, B), dim3(512), a))); break;
        case Core::C512: CHK((step_launch<&k_clip_attn_w<8, 10, 2>>(h, dim3(4, B), dim3(512), a))); break;
        default: return no_inst(h, "k_clip_attn_w");
    }
    const FfnArgs f = ffn_args(h, y, true);
    // latent_dim 384: W_o (36 fragments per wave) waits in registers as at the ZEGGS widths; 512: 64 fragments do not fit -- W_o leads the weight ring.
    // Round 6: with >= 3 lanes whose row tiles together need more than one round of the 256 CUs, 32-row blocks -- W_o | W1 | W2 (1.8 / 2.5 MB) streamed once
    // per 32 rows; W_o leads the ring at both widths (20 / 12 slots: 250 VGPRs), at 512 the fp32 LayerNorm1 rows wait in X1 instead of the LDS.
    // Bit-identical to the 16-row form.  BEAT 4 x 16 clips 946 -> 825 us per step, 4 x 8: 542 -> 516; 1 x 16: 375 -> 412, 4 x 4: 375 -> 398, 2 x 16 even
    // (profiles/r06_dj_*)
    const bool rows32 = y.ks.ffn_rows == 32;
    switch (h->core) {
        case Core::C384:
            if (rows32) return step_launch<&k_ffn<P, 6, 16, 2, 8, 2, true, true, 20, true>>(h, dim3(cdiv(MT, 2)), dim3(512), f);
            return step_launch<&k_ffn<P, 6, 16, 1, 8, 2, true, true, 24>>(h, dim3(MT), dim3(512), f);      // (W_o leading the ring here too: 353.1 -> 357.8 us per step at 16 clips, r06_ea)
        case Core::C512:
            if (rows32) return step_launch<&k_ffn<P, 8, 16, 2, 8, 2, true, true, 12, true>>(h, dim3(cdiv(MT, 2)), dim3(512), f);
            return step_launch<&k_ffn<P, 8, 16, 1, 8, 2, true, true, 24, true>>(h, dim3(MT), dim3(512), f);
        default: return no_inst(h, "k_ffn<OP>");
    }
}
// ROWS at the DSG+ widths in bf16w2: the QKV GEMM on the hi + lo rows in X0a (layer 0: the embedding, after it LayerNorm2 of the previous layer), k_attn -- its rows
// are the fragment-major pair k_ffn<OP> takes -- and k_ffn<OP> on one 16-row tile: W_o | W1 | W2 as two-register fragments through a 16-slot ring, the attention
// rows / LayerNorm1 rows re-read from their LDS image per k-block (A_LDS; held they are 96 / 128 registers)
template <class P>
static int layer_qkv_attn_ffn(dsg_handle* h, const LayerCtx& y) {
    GemmArgs g = gemm_qkv(h, y.z, y.M, y.ly, 1, nullptr);
    g.KS = 1; g.kb_per_split = g.KBtot;
    g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
    if (g.NT % 4) return fail(DSG_E_INVALID, "gemm: NT not divisible by the workgroup tile");
    const dim3 grid(xcd_grid_x(g.NT / 4), g.MT, 1);
    switch (h->core) {      // (one batch of fragment loads per wave: 12 / 16 k-blocks)
        case Core::C384: CHK((step_launch<&k_gemm_qkv_pair<P, 12>>(h, grid, dim3(256), g))); break;
        case Core::C512: CHK((step_launch<&k_gemm_qkv_pair<P, 16>>(h, grid, dim3(256), g))); break;
        default: return no_inst(h, "k_gemm_qkv_pair");
    }
    CHK(launch_attn<P>(h, y.z.B));
    const FfnArgs f = ffn_args(h, y, true);
    switch (h->core) {
        case Core::C384: return step_launch<&k_ffn<P, 6, 16, 1, 8, 2, true, true, 16, true, true>>(h, dim3(y.MT), dim3(512), f);
        case Core::C512: return step_launch<&k_ffn<P, 8, 16, 1, 8, 2, true, true, 16, true, true>>(h, dim3(y.MT), dim3(512), f);
        default: return no_inst(h, "k_ffn<OP>");
    }
}
// the forms that exist for precision P (select_kernels picks no other): fp32 has no k_clip_attn / k_ffn, bf16w2 no k_attn_op
template <class P>
static int run_layer(dsg_handle* h, Form f, const LayerCtx& y) {
    constexpr bool bf16 = std::is_same<P, PBF16>::value;
    switch (f) {
        case Form::MID: return layer_mid<P>(h, y);
        case Form::UNFUSED: return layer_unfused<P>(h, y);
        case Form::ATTN_OP: if constexpr (!P::W2) return layer_attn_op<P>(h, y); break;
        case Form::ATTN_OP_SPLIT: if constexpr (!P::W2) return layer_attn_op_split<P>(h, y); break;
        case Form::CLIP_SPLIT: if constexpr (bf16) return layer_clip_split<P>(h, y); break;
        case Form::ATTN_OP_FFN: if constexpr (bf16) return layer_attn_op_ffn<P>(h, y); break;
        case Form::CLIP_FFN: if constexpr (bf16 || P::W2) return layer_clip_ffn<P>(h, y); break;
        case Form::CLIP_W_FFN: if constexpr (bf16) return layer_clip_w_ffn<P>(h, y); break;
        case Form::QKV_ATTN_FFN: if constexpr (P::W2) return layer_qkv_attn_ffn<P>(h, y); break;
    }
    return fail(DSG_E_NOT_IMPLEMENTED, "layer form without an instantiation for this precision");
}

template <class P>
static int run_step(dsg_handle* h, const StepCtx& c) {
    const int B = c.B, D = h->D, T = h->T, ntok = h->ntok;
    const int Min = B * T, M = B * ntok, MT = cdiv(M, 16);
    const KernelSel& ks = c.ks;
    StepCtl* const ctl = c.use_ctr ? h->ctl : nullptr;
    const GemmArgs z = gemm_base(h, B);
    const LocArgs la = loc_args(h, B, ks.ks_in, ctl, ks.x0a_frag);
    h->fence_next = 1;         // the first packet of a step reads the state the previous step's last packet wrote (state_fences)
    if (ks.set == DSG_KSET_LATENCY) {      // pose embedding + local attention in one launch (in the batched sets it loses: 1 x 16 clips 192.1 -> 198.5 us
                                           // per step, 1 x 64: 258 -> 291, 4 x 4 even -- profiles/r06_ab_*, round 6)
        CHK((launch_loc<P, true, 256>(h, dim3(h->Hl, T / h->W, B + 1), inloc_args(h, la, ctl, h->n_run))));
    } else {
        {
            GemmArgs g = gemm_pose_in(h, z, Min, ks.ks_in);
            step_ctl(h, g, ctl);
            bool done = false;
            if constexpr (sizeof(typename P::elem) == 2 && !P::W2) {
                if (ks.xs_frag) { g.a_frag = 1; CHK(launch_ws2<EPI_PARTIAL>(h, g)); done = true; }      // the state shadow is fragment-major
            }
            if constexpr (!P::W2) {
                if (!done && ks.blk()) { CHK((launch_blk_k<P, EPI_PARTIAL>(h, g))); done = true; }
            }
            if (!done) CHK((launch_gemm<P, PRO_DIRECT, EPI_PARTIAL, 4, 1>(h, g)));
        }
        // Round 6: from 2048 (head, window, clip) items TWO waves each instead of a 256-thread workgroup: the kernel is one ~5 us chain of dependent
        // phases per item, and 4096 workgroups of 4 waves (64 clips) need two rounds of the CUs' 8 workgroup slots where 4096 x 2 waves are all
        // resident at once (32 per CU) -- 1 x 64 clips 249.1 -> 245.0 us per step (one wave each: 246.4), 4 x 64: 705 -> 692-702 (29.2-29.6 k frames/s);
        // k_loc itself 13.3 -> 10.0 us at 5696 rows with one wave; below 2048 items the 4-wave form is ahead (16 clips: 184.1 vs 186.0).  Same arithmetic
        // (the matrix-instruction tail is one wave's work in every form): bit-identical.  profiles/r06_cj_*, r06_cl_*
        if (h->Hl * (T / h->W) * B >= h->env_loc64_from) CHK((launch_loc<P, false, 128>(h, dim3(h->Hl, T / h->W, B), la)));
        else CHK((launch_loc<P, false, 256>(h, dim3(h->Hl, T / h->W, B), la)));
    }
    int in_frag = ks.x0a_frag;
    for (int l = 0; l < h->L; ++l) {
        const Form f = layer_form(h, ks, l);
        const LayerCtx y = {ks, z, h->layers[l], M, MT, l == 0 ? h->X0 : h->Xn, in_frag, l == 0 ? nullptr : &h->layers[l - 1]};
        CHK(run_layer<P>(h, f, y));
        in_frag = leaves_x0a(f) ? 1 : -1;
    }
    {   // final LayerNorm-on-read + pose head + sampler update
        GemmArgs g = gemm_pose_head(h, z, M, h->layers[h->L - 1]);
        step_ctl(h, g, ctl);
        g.out_mode = c.out_mode; g.ext_noise = c.ext_noise; g.const_noise = c.const_noise; g.keyed = c.keyed; g.clip_x0 = c.clip_x0; g.no_noise = c.no_noise;
        g.xs_frag = ks.xs_frag ? 1 : 0;
        if (c.inpaint) { g.inp32 = h->inp32; g.inp_mask = h->inp_mask; }      // every pose-head form below reads the same GemmArgs
        h->fence_next = 2;     // the last packet of a step writes the state (state_fences)
        if (h->cfgB > 0) {      // guidance: one workgroup per CONDITIONAL row tile evaluates the twin rows as well (k_gemm_cfg; ROWS at the DSG+ widths: k_ws_cfg)
            g.B = h->cfgB; g.M = h->cfgB * ntok; g.MT = cdiv(g.M, 16);
            g.cfgB = h->cfgB; g.cfg_off = h->cfgB * ntok; g.cfg_scale = h->cfg_scale;
            g.KS = 1; g.kb_per_split = g.KBtot; g.inv_ntok = fastdiv_inv(g.ntok); g.inv_hd = fastdiv_inv(g.hd);
            if (cfg_head_streams(ks.form)) {      // the last layer kept the set's form: its LayerNorm2 rows (+ twins) lie fragment-major in X0a (k_ws_cfg)
                if constexpr (sizeof(typename P::elem) == 2 && !P::W2) {
                    g.X = nullptr; g.ln_g = nullptr; g.ln_b = nullptr; g.A = h->X0a; g.lda = D; g.a_frag = 1;
                    CHK(launch_ws_cfg(h, g));
                } else {
                    return fail(DSG_E_NOT_IMPLEMENTED, "guided pose head on the rows in X0a: bf16 only");
                }
            } else {
                if (g.NT % 4) return fail(DSG_E_INVALID, "gemm: NT not divisible by the workgroup tile");
                const dim3 grid(xcd_grid_x(g.NT / 4), g.MT + 1, 1);
                // (bf16w2: 16 k-blocks of two-register weight + activation fragments do not fit -- two batches of 8, as in launch_gemm_w; round-5 advisor)
                bool done = false;
                if constexpr (!P::W2) {
                    if (pick_ch(g.KBtot) == 16) { CHK((step_launch<&k_gemm_cfg<P, 16>>(h, grid, dim3(256), g))); done = true; }
                }
                if (!done && pick_ch(g.KBtot) == 12) { CHK((step_launch<&k_gemm_cfg<P, 12>>(h, grid, dim3(256), g))); done = true; }
                if (!done) CHK((step_launch<&k_gemm_cfg<P>>(h, grid, dim3(256), g)));
            }
        } else if (leaves_x0a(ks.form)) {      // the last layer left its rows normalised in X0a (no guidance here)
            g.X = nullptr; g.ln_g = nullptr; g.ln_b = nullptr; g.A = h->X0a; g.lda = D; g.a_frag = 1;
            CHK((launch_gemm_w<P, PRO_DIRECT, EPI_OUT>(h, g, ks)));
        } else {
            CHK((launch_gemm_w<P, PRO_LN, EPI_OUT>(h, g, ks)));
        }
    }
    return 0;
}
// ---- diagnostics: time a chain of ONE phase kernel (graph replay) to separate launch floor, kernel body and
//      weight coldness.  which: 0 null, 1 out_proj GEMM of layer 0 (same weights every launch), 2 out_proj cycling
//      over the layers, 3 LN+linear1+GELU cycling, 4 linear2 cycling, 5 k_attn, 6 k_loc, 7 k_in, 8 pose head (forward),
//      9 LN+QKV cycling, 10 k_mid cycling, 12 k_inloc
template <class P>
static int debug_launch(dsg_handle* h, int which, int i, int B) {
    const int T = h->T, M = B * h->ntok;
    const GemmArgs z = gemm_base(h, B);
    const Layer& ly = h->layers[(which == 1) ? 0 : i % h->L];
    const LocArgs la = loc_args(h, B, h->KSin, nullptr, 0);
    if (which == 20) return debug_launch<P>(h, (i & 1) ? 1 : 4, i, B);                 // alternate 2 kernels
    if (which == 21) { const int seq[4] = {1, 4, 7, 9}; return debug_launch<P>(h, seq[i & 3], i, B); }   // 4 kernels
    if (which == 22) { const int seq[6] = {12, 9, 5, 10, 4, 8}; return debug_launch<P>(h, seq[i % 6], i, B); } // the step's 6 kernels
    // the step's own GemmArgs (gemm_*), every GEMM on the 16 x 16 tile kernel; what a chain of one kernel changes is set after the builder call
    switch (which) {
        case 0: hipLaunchKernelGGL(k_ctr_inc, dim3(96), dim3(256), 0, h->stream, h->ctr); return 0;
        case 1: case 2: {
            GemmArgs g = gemm_out_proj(h, z, M, ly, h->X0);
            g.out = (i & 1) ? h->pre1 : h->pre2;      // (two targets in turn)
            return launch_gemm<P, PRO_DIRECT, EPI_RESID, 4, 1>(h, g); }
        case 3: return launch_gemm<P, PRO_LN, EPI_GELU, 4, 1>(h, gemm_linear1(h, z, M, ly, false));
        case 4: return launch_gemm<P, PRO_DIRECT, EPI_RESID, 1, 4>(h, gemm_linear2(h, z, M, ly));
        case 5: return launch_attn<P>(h, B);
        case 6: return launch_loc<P, false, 256>(h, dim3(h->Hl, T / h->W, B), la);
        case 7: return launch_gemm<P, PRO_DIRECT, EPI_PARTIAL, 4, 1>(h, gemm_pose_in(h, z, B * T, h->KSin));      // (no control block: the step does not advance)
        case 8: {
            GemmArgs g = gemm_pose_head(h, z, M, ly);
            g.out_mode = OUT_FORWARD; g.xsA = nullptr;      // a forward: writes fwd_out, leaves the state and its shadow alone
            g.st = step_tables(h); g.n_tab = 1;             // ... and reads no control block
            return launch_gemm<P, PRO_LN, EPI_OUT, 4, 1>(h, g); }
        case 9: return launch_gemm<P, PRO_LN, EPI_QKV, 4, 1>(h, gemm_qkv(h, z, M, ly, -1, &ly));      // (LayerNorm2 of the same layer)
        case 10: return launch_mid<P>(h, mid_args(h, ly, h->Xn, M));
        case 12: return launch_loc<P, true, 256>(h, dim3(h->Hl, T / h->W, B + 1), inloc_args(h, la, nullptr, 1));
        default: return fail(DSG_E_INVALID, "debug_chain: unknown kernel id");
    }
}
// copies an internal buffer to the host (raw bytes) -- used to bisect GPU-vs-emulator differences
extern "C" int dsg_debug_read(dsg_handle* h, const char* name, void* out, long long max_bytes, long long* n_bytes) {
    if (!h || !name || !out) return fail(DSG_E_INVALID, "null");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t B = h->Bmax, D = h->D, M = rup((int)(B * h->ntok), 16), Min = rup((int)(B * h->T), 16), es = h->es;
    std::map<std::string, std::pair<const void*, size_t>> m = {
        {"partial", {h->partial, (size_t)h->KSin * Min * D * 4}}, {"X0", {h->X0, M * D * 4}}, {"X0a", {h->X0a, M * D * es}},
        {"q", {h->q, B * h->H * h->Tp * h->hd * es}}, {"k", {h->k, B * h->H * h->Tp * h->hd * es}},
        {"vt", {h->vt, B * h->H * h->Tp * h->hd * es}}, {"attn", {h->attn, M * D * es}}, {"pre1", {h->pre1, M * D * 4}},
        {"X1", {h->X1, M * D * 4}}, {"Xn", {h->Xn, M * D * 4}}, {"hidden", {h->hidden, M * h->ff * es}},
        {"pre2", {h->pre2, M * D * 4}}, {"fwd_out", {h->fwd_out, B * h->J * h->T * 4}},
        {"xs32", {h->xs32, B * h->T * h->Jp * 4}}, {"xsA", {h->xsA, h->xsA ? Min * h->Jp * es : 0}},
        {"Cf", {h->Cf, B * h->T * D * 4}}, {"emb1", {h->emb1, B * D * 4}}};
    auto it = m.find(name);
    if (it == m.end() || !it->second.first) return fail(DSG_E_INVALID, "unknown buffer");
    size_t n = std::min<size_t>(it->second.second, (size_t)max_bytes);
    HIPCHK(hipMemcpy(out, it->second.first, n, hipMemcpyDeviceToHost));
    if (n_bytes) *n_bytes = (long long)n;
    return 0;
}

extern "C" int dsg_debug_chain(dsg_handle* h, int which, int n, int use_graph, int B, float* us_per_launch) {
    if (!h || !h->finalized || !h->cond_set) return fail(DSG_E_STATE, "debug_chain needs a finalized, conditioned handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->prec == DSG_PREC_BF16W2) return fail(DSG_E_NOT_IMPLEMENTED, "dsg_debug_chain: precision bf16w2");
#ifdef DSG_DEV_BF16_ONLY
    auto one = [&](int i) { return debug_launch<PBF16>(h, which, i, B); };
#else
    auto one = [&](int i) { return h->prec == DSG_PREC_BF16 ? debug_launch<PBF16>(h, which, i, B) : debug_launch<PF32>(h, which, i, B); };
#endif
    const int G = 64;
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    if (use_graph) {
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < G; ++i) CHK(one(i));
        HIPCHK(hipStreamEndCapture(h->stream, &graph));
        HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    }
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        HIPCHK(hipEventRecord(h->ev_t0, h->stream));
        if (use_graph) for (int i = 0; i < n / G; ++i) HIPCHK(hipGraphLaunch(exec, h->stream));
        else for (int i = 0; i < n; ++i) CHK(one(i));
        HIPCHK(hipEventRecord(h->ev_t1, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        float ms; HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
        best = std::min(best, 1000.f * ms / (use_graph ? (n / G) * G : n));
    }
    if (exec) { (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph); }
    *us_per_launch = best;
    return 0;
}

// ---- diagnostics: per-packet timeline of the AQL step loop (dsg_aql.h: Trace).  dsg_debug_trace_arm before a dsg_sample traces
//      steps [first, first + n) of that call; dsg_debug_trace_get returns, per traced step and packet, start / end in us (relative
//      to the first traced dispatch) + the kernel names, ';'-separated.
extern "C" int dsg_debug_trace_arm(dsg_handle* h, int first, int n) {
    if (!h || first < 0 || n <= 0) return fail(DSG_E_INVALID, "dsg_debug_trace_arm: bad argument");
#ifndef DSG_EMU
    h->aql.trace.armed = true; h->aql.trace.first = first; h->aql.trace.n = n;
    return 0;
#else
    return fail(DSG_E_NOT_IMPLEMENTED, "no AQL path under emulation");
#endif
}
extern "C" int dsg_debug_trace_get(dsg_handle* h, double* us, int cap, int* n_steps, int* n_packets, char* names, int names_cap) {
    if (!h || !us || !n_steps || !n_packets) return fail(DSG_E_INVALID, "null argument");
#ifndef DSG_EMU
    const dsg_aql::Trace& t = h->aql.trace;
    const int L = (int)t.names.size();
    if (L == 0 || t.us.empty()) return fail(DSG_E_STATE, "no trace: arm it, then sample through the AQL path");
    *n_packets = L; *n_steps = (int)(t.us.size() / 2 / L);
    if ((int)t.us.size() > cap) return fail(DSG_E_INVALID, "trace buffer too small");
    memcpy(us, t.us.data(), t.us.size() * sizeof(double));
    if (names && names_cap > 0) {
        std::string all;
        for (const auto& n : t.names) { all += n; all += ';'; }
        snprintf(names, (size_t)names_cap, "%s", all.c_str());
    }
    return 0;
#else
    return fail(DSG_E_NOT_IMPLEMENTED, "no AQL path under emulation");
#endif
}

// marks build (-DDSG_STAMPS=2): per traced step, packet and mark k < 12: {waves that passed the mark, mean, last wave} in us after the packet's
// first wave start (dsg_kernels.h: DSG_TL_MARK)
extern "C" int dsg_debug_trace_marks(dsg_handle* h, double* out, int cap, int* n_marks) {
    if (!h || !out || !n_marks) return fail(DSG_E_INVALID, "null argument");
#if !defined(DSG_EMU) && defined(DSG_STAMPS) && DSG_STAMPS >= 2
    const dsg_aql::Trace& t = h->aql.trace;
    if (t.marks.empty()) return fail(DSG_E_STATE, "no marks: arm a trace, then sample through the AQL path");
    if ((int)t.marks.size() > cap) return fail(DSG_E_INVALID, "marks buffer too small");
    memcpy(out, t.marks.data(), t.marks.size() * sizeof(double));
    *n_marks = DSG_TL_NMARK;
    return 0;
#else
    (void)cap;
    return fail(DSG_E_NOT_IMPLEMENTED, "phase marks exist in the marks build only (make marks)");
#endif
}

static int run_step_p(dsg_handle* h, const StepCtx& c) {
#ifndef DSG_DEV_BF16_ONLY
    if (h->prec == DSG_PREC_BF16W2) return run_step<PBF16W2>(h, c);
    if (h->prec == DSG_PREC_FP32) return run_step<PF32>(h, c);
#endif
    return run_step<PBF16>(h, c);
}

// the launch of a kernel that walks the state's [B][T][Jp / 4] quads grid-stride (the start kernels, the hand-offs, the constraint cuts)
template <class Args>
static int launch_state(dsg_handle* h, void (*kernel)(Args), int B, const Args& a) {
    const size_t n = (size_t)B * h->T * (h->Jp / 4);
    hipLaunchKernelGGL(kernel, dim3((int)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_x_in(dsg_handle* h, const float* x, const float* init, int do_q, float qa, float qb, int use_philox,
                       NoiseKey nk, const unsigned* keys, const unsigned* offs, unsigned draw, int B, const KernelSel& ks) {
    XInArgs a;
    a.keys = keys; a.offs = offs;
    a.dupB = h->cfgB; a.xs_frag = ks.xs_frag ? 1 : 0;
    a.x = x; a.init = init; a.do_q = do_q; a.qa = qa; a.qb = qb; a.use_philox = use_philox; a.nkey = nk; a.draw = draw;
    a.B = B; a.J = h->J; a.Jp = h->Jp; a.Jq = h->Jq; a.T = h->T; a.xs32 = h->xs32;
    a.xsA = is_bf16(h) ? h->xsA : nullptr;
    return launch_state(h, is_bf16(h) ? k_x_in<PBF16> : k_x_in<PF32>, B, a);
}
// window c of a clip of n_out frames that starts from the handle's clip-level init motion (dsg_sample_clip): cut + q_sample + state write
static ClipXInArgs clip_x_in_args(dsg_handle* h, int c, int n_out, float qa, float qb, NoiseKey nk, const unsigned* keys, const unsigned* offs,
                                  unsigned draw, int B, const KernelSel& ks) {
    ClipXInArgs a;
    a.keys = keys; a.offs = offs;
    a.init = h->cinit_motion; a.c_seed = h->c_seed; a.qa = qa; a.qb = qb; a.nkey = nk; a.draw = draw;
    a.B = B; a.J = h->J; a.Jp = h->Jp; a.Jq = h->Jq; a.T = h->T; a.S = h->S; a.n_out = n_out; a.c = c;
    a.xs32 = h->xs32; a.xsA = is_bf16(h) ? h->xsA : nullptr;
    a.dupB = h->cfgB; a.xs_frag = ks.xs_frag ? 1 : 0;
    return a;
}
static int launch_clip_x_in(dsg_handle* h, int c, int n_out, float qa, float qb, NoiseKey nk, const unsigned* keys, const unsigned* offs,
                            unsigned draw, int B, const KernelSel& ks) {
    const ClipXInArgs a = clip_x_in_args(h, c, n_out, qa, qb, nk, keys, offs, draw, B, ks);
    return launch_state(h, is_bf16(h) ? k_clip_x_in<PBF16> : k_clip_x_in<PF32>, B, a);
}
// a round of dsg_sample_clip_queue_edit on a lane that runs a job with an init motion: init, length and window index per slot (h->cq.edits)
static int launch_clip_x_in_q(dsg_handle* h, NoiseKey nk, const unsigned* keys, const unsigned* offs, unsigned draw, int B, const KernelSel& ks) {
    ClipXInQArgs a;
    a.x = clip_x_in_args(h, 0, 0, 0.f, 0.f, nk, keys, offs, draw, B, ks);
    a.x.init = nullptr;      // (per slot, from the table, as n_out, c, do_q and the q_sample pair)
    a.slots = h->cq.edits;
    return launch_state(h, is_bf16(h) ? k_clipq_x_in<PBF16> : k_clipq_x_in<PF32>, B, a);
}
static int launch_x_out(dsg_handle* h, float* dst_dev, int B) {
    const size_t n = (size_t)B * h->J * h->T;
    hipLaunchKernelGGL(k_x_out, dim3((int)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, h->stream, h->xs32,
                       dst_dev, B, h->J, h->Jp, h->T);
    HIPCHK(hipGetLastError());
    return 0;
}

// `user_stream` is the caller's hipStream_t; NULL is the legacy default stream (torch's default on ROCm), which does
// NOT implicitly synchronise with the handle's non-blocking stream -- so the ordering events are always recorded.
static int order_after(dsg_handle* h, void* user_stream) {
    HIPCHK(hipEventRecord(h->ev_in, (hipStream_t)user_stream));
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
    return 0;
}
static int order_before(dsg_handle* h, void* user_stream) {
    HIPCHK(hipEventRecord(h->ev_out, h->stream));
    HIPCHK(hipStreamWaitEvent((hipStream_t)user_stream, h->ev_out, 0));
    return 0;
}
// bring a caller tensor to the device (returns the device pointer to use)
static int to_dev(dsg_handle* h, const float* src, float* staging, size_t n, const float** out) {
    if (!src) { *out = nullptr; return 0; }
    if (is_device_ptr(src)) { *out = src; return 0; }
    HIPCHK(hipMemcpyAsync(staging, src, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *out = staging;
    return 0;
}
static int from_dev(dsg_handle* h, float* dst, const float* src_dev, size_t n) {
    if (is_device_ptr(dst)) {
        HIPCHK(hipMemcpyAsync(dst, src_dev, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    } else {
        HIPCHK(hipMemcpyAsync(dst, src_dev, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// rows the kernels run on for a user batch of B (guidance doubles it); checks B against the conditioning
static int rows_for(dsg_handle* h, int B, int* rows) {
    const int want = h->cfgB > 0 ? h->cfgB : h->condB;
    if (B != want) return fail(DSG_E_INVALID, "batch differs from the batch of dsg_set_window_cond");
    *rows = h->condB;
    return 0;
}

// y['inpainting_mask'] / y['inpainted_motion'] of the sampling loops (main/diffusion/gaussian_diffusion.py:317-321): both [B, J, 1, T], host or
// device.  Every step of dsg_sample / dsg_sample_multi then replaces the model's x0 prediction -- after the guidance combination, before the
// clamp and the posterior -- by the motion wherever the mask is set (GemmArgs::inp32).  Sticky until switched off (both NULL); the window
// conditioning does not touch it.  The constraint is kept in the state's layout, in cached memory like the conditioning: the loop only reads it.
extern "C" int dsg_set_inpainting(dsg_handle* h, const uint8_t* mask, const float* motion, int B, void* stream) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    CHK(owned_by_queue(h));
    if (!mask && !motion) { h->inpB = 0; return 0; }
    if (!mask || !motion) return fail(DSG_E_INVALID, "dsg_set_inpainting: mask and motion go together (both NULL switches the constraint off)");
    if (B <= 0 || B > h->Bmax) return fail(DSG_E_INVALID, "batch exceeds max_batch");
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t n = (size_t)B * h->J * h->T, nq = (size_t)B * h->T * (h->Jp / 4);
    // (each pointer on its own: a call that failed half way through leaves the rest to the next one)
    if (!h->inp32) CHK(dalloc(h, &h->inp32, (size_t)h->Bmax * h->T * h->Jp));
    if (!h->inp_mask) CHK(dalloc(h, &h->inp_mask, (size_t)h->Bmax * h->T * h->Jp));
    if (!h->inp_stage) CHK(dalloc(h, &h->inp_stage, (size_t)h->Bmax * h->J * h->T));
    CHK(order_after(h, stream));
    const float* md = nullptr;
    CHK(to_dev(h, motion, h->io_tmp, n, &md));
    const uint8_t* kd = mask;
    if (!is_device_ptr(mask)) {
        HIPCHK(hipMemcpyAsync(h->inp_stage, mask, n, hipMemcpyHostToDevice, h->stream));
        kd = h->inp_stage;
    }
    hipLaunchKernelGGL(k_inp_in, dim3((int)std::min<size_t>((nq + 255) / 256, 2048)), dim3(256), 0, h->stream, md, kd, B, h->J, h->Jp, h->T,
                       h->inp32, h->inp_mask);
    HIPCHK(hipGetLastError());
    h->inpB = B;
    CHK(order_before(h, stream));
    return 0;
}

// The constraint of a whole clip, for dsg_sample_clip / _multi: mask uint8 / motion fp32 [B, n_frames, J] in the coordinates of the stitched
// clip (frame-major, the layout and frame numbering of dsg_sample_clip's `out`), host or device.  The library keeps its own copy (the caller's
// buffers are free once `stream` has passed the call) and cuts every window's constraint out of it on the device (k_clip_inp_window) into the
// buffers of dsg_set_inpainting, which are allocated here too.  Sticky until switched off (both NULL); dsg_forward / dsg_sample / _multi ignore it.
extern "C" int dsg_set_clip_inpainting(dsg_handle* h, const uint8_t* mask, const float* motion, int B, int n_frames, void* stream) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    CHK(owned_by_queue(h));
    if (!mask && !motion) { h->cinpB = 0; h->cinp_frames = 0; return 0; }
    if (!mask || !motion) return fail(DSG_E_INVALID, "dsg_set_clip_inpainting: mask and motion go together (both NULL switches the constraint off)");
    if (B <= 0 || B > h->Bmax) return fail(DSG_E_INVALID, "batch exceeds max_batch");
    if (n_frames < 1) return fail(DSG_E_INVALID, "dsg_set_clip_inpainting: n_frames < 1");
    HIPCHK(hipSetDevice(h->cfg.device));
    h->cinpB = 0; h->cinp_frames = 0;      // (a call that fails below leaves the constraint off, not half written)
    const size_t n = (size_t)B * n_frames * h->J;
    if (n > h->cinp_cap) {
        h->cinp_cap = 0;
        CHK(regrow(h, &h->cinp_motion, n));
        CHK(regrow(h, &h->cinp_mask, n));
        h->cinp_cap = n;
    }
    // (each pointer on its own, as dsg_set_inpainting)
    if (!h->inp32) CHK(dalloc(h, &h->inp32, (size_t)h->Bmax * h->T * h->Jp));
    if (!h->inp_mask) CHK(dalloc(h, &h->inp_mask, (size_t)h->Bmax * h->T * h->Jp));
    CHK(order_after(h, stream));
    CHK(upload(h, h->cinp_motion, motion, n * sizeof(float)));
    CHK(upload(h, h->cinp_mask, mask, n));
    h->cinpB = B; h->cinp_frames = n_frames;
    CHK(order_before(h, stream));
    return 0;
}

// The motion a whole clip is re-denoised from, for dsg_sample_clip / _multi (init_image of every window of the loop, gaussian_diffusion.py:
// 701-713): motion fp32 [B, n_frames, J] in the coordinates of the stitched clip, host or device.  The library keeps its own copy (the caller's
// buffer is free once `stream` has passed the call); every window starts from q_sample of its slice (k_clip_x_in).  Sticky until switched off
// (NULL); dsg_forward / dsg_sample / _multi ignore it.
extern "C" int dsg_set_clip_init(dsg_handle* h, const float* motion, int B, int n_frames, void* stream) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    CHK(owned_by_queue(h));
    if (!motion) { h->cinitB = 0; h->cinit_frames = 0; return 0; }
    if (B <= 0 || B > h->Bmax) return fail(DSG_E_INVALID, "batch exceeds max_batch");
    if (n_frames < 1) return fail(DSG_E_INVALID, "dsg_set_clip_init: n_frames < 1");
    HIPCHK(hipSetDevice(h->cfg.device));
    h->cinitB = 0; h->cinit_frames = 0;      // (a call that fails below leaves it off, not half written)
    const size_t n = (size_t)B * n_frames * h->J;
    if (n > h->cinit_cap) {
        h->cinit_cap = 0;
        CHK(regrow(h, &h->cinit_motion, n));
        h->cinit_cap = n;
    }
    CHK(order_after(h, stream));
    CHK(upload(h, h->cinit_motion, motion, n * sizeof(float)));
    h->cinitB = B; h->cinit_frames = n_frames;
    CHK(order_before(h, stream));
    return 0;
}

// Per-element noise streams ("keyed noise") for dsg_sample / _multi / dsg_sample_clip / _multi: element b of the batch draws from
// (seeds[b], stream_ids[b]) with the batch term of the Philox counter 0 -- draw d at (f, j) = philox4x32_10(ctr = ((f Jq + j) >> 2, d,
// sid_b lo, sid_b hi), key = (seed_b lo, seed_b hi)) + Box-Muller, the [1, J, 1, T] tensor of its pair -- so its noise is exactly the noise it
// gets sampled alone (B = 1) with args->seed = seeds[b], args->stream_id = stream_ids[b], whichever batch, slot and lane it rides in.  Draw
// indices stay per call (draw_base, draw_base + 1 + i, a clip's window c from draw_base + c (1 + n_run)).  Host arrays, copied here; the
// table reaches the device with the `dyn` block of every sampling call (sample_prepare).  Reference counterpart: none (th.randn consumes one
// global generator, gaussian_diffusion.py:704, :542).
static void set_noise_key(unsigned* key, uint64_t seed, uint64_t stream_id) {      // an element's entry of a key table
    key[0] = (unsigned)(seed & 0xffffffffu); key[1] = (unsigned)(seed >> 32);
    key[2] = (unsigned)(stream_id & 0xffffffffu); key[3] = (unsigned)(stream_id >> 32);
}
extern "C" int dsg_set_noise_streams(dsg_handle* h, const uint64_t* seeds, const uint64_t* stream_ids, int B) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    CHK(owned_by_queue(h));
    if (!seeds && !stream_ids) { h->nkB = 0; return 0; }
    if (B < 1 || B > h->Bmax)
        return fail(DSG_E_INVALID, "dsg_set_noise_streams: batch " + std::to_string(B) + " outside 1 .. max_batch (" + std::to_string(h->Bmax) + ")");
    h->nkeys.assign(4 * (size_t)B, 0u);
    for (int b = 0; b < B; ++b) set_noise_key(&h->nkeys[4 * b], seeds ? seeds[b] : 0, stream_ids ? stream_ids[b] : 0);
    h->nk_seeds = seeds != nullptr;
    h->nkB = B;
    return 0;
}

extern "C" int dsg_forward(dsg_handle* h, const float* x, const int64_t* t, float* out, int B, void* stream) {
    if (!h || !x || !t || !out) return fail(DSG_E_INVALID, "dsg_forward: null argument");
    CHK(owned_by_queue(h));
    if (!h->finalized || !h->cond_set) return fail(DSG_E_STATE, "dsg_forward before finalize / set_window_cond");
    int rows = 0;
    CHK(rows_for(h, B, &rows));
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(order_after(h, stream));
    std::vector<int> tt(rows);
    if (is_device_ptr(t)) {
        std::vector<int64_t> th(B);
        HIPCHK(hipMemcpy(th.data(), t, B * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) tt[i] = (int)th[i];
    } else {
        for (int i = 0; i < B; ++i) tt[i] = (int)t[i];
    }
    for (int i = B; i < rows; ++i) tt[i] = tt[i - B];      // guidance: the twins share the timestep
    for (int i = 0; i < B; ++i)
        if (tt[i] < 0 || tt[i] >= h->n_te) return fail(DSG_E_INVALID, "timestep out of range");
    HIPCHK(hipMemcpyAsync(h->t_arr, tt.data(), rows * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));     // tt is a stack-lifetime staging buffer
    const size_t n = (size_t)B * h->J * h->T;
    const float* xd = nullptr;
    CHK(to_dev(h, x, h->io_tmp, n, &xd));
    NoiseKey nk = {0, 0, 0, 0};
    StepCtx c; c.B = rows; c.out_mode = OUT_FORWARD; c.use_ctr = false; c.ext_noise = nullptr; c.const_noise = 0;
    CHK(select_kernels(h, rows, 1, c.ks));
    CHK(ensure_set_buffers(h, c.ks));
    CHK(launch_x_in(h, xd, nullptr, 0, 0.f, 0.f, 0, nk, nullptr, nullptr, 0, B, c.ks));
    CHK(run_step_p(h, c));
    h->last.kset = c.ks.set;      // (no sampling call: the rest of the report stays)
    CHK(from_dev(h, out, h->fwd_out, n));
    CHK(order_before(h, stream));
    return 0;
}

// per-step coefficient tables in execution order (gaussian_diffusion.py:1617 `.float()` of the float64 tables)
static int build_step_tables(dsg_handle* h, int mode, int skip, float eta, int* n_run_out) {
    const Sched& s = h->sched;
    if (s.n == 0) return fail(DSG_E_STATE, "dsg_sample before dsg_set_schedule");
    if (skip < 0 || skip >= s.n) return fail(DSG_E_INVALID, "skip_timesteps out of range");
    const int n_run = s.n - skip;
    // every window of a clip asks for the same tables: they stay on the device until schedule / mode / skip / eta change
    if (h->st_valid && h->st_mode == mode && h->st_skip == skip && h->st_eta == eta) {
        *n_run_out = n_run; h->n_run = n_run;
        return 0;
    }
    std::vector<int> tm(n_run);
    std::vector<float> c[5];
    for (auto& v : c) v.assign(n_run, 0.f);
    for (int i = 0; i < n_run; ++i) {
        const int idx = n_run - 1 - i;
        tm[i] = s.tmap[idx];
        const float nz = idx == 0 ? 0.f : 1.f;
        if (mode == DSG_MODE_DDPM) {
            c[0][i] = (float)s.coef1[idx];
            c[1][i] = (float)s.coef2[idx];
            c[2][i] = nz * expf(0.5f * (float)s.plogvar[idx]);
        } else {
            const float ab = (float)s.ac[idx], abp = (float)s.acp[idx];
            const float sigma = eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
            c[0][i] = (float)s.sqrt_recip[idx];
            c[1][i] = (float)s.sqrt_recipm1[idx];
            c[2][i] = sqrtf(abp);
            c[3][i] = sqrtf(1.f - abp - sigma * sigma);
            c[4][i] = nz * sigma;
        }
    }
    HIPCHK(hipMemcpyAsync(h->st_tmodel, tm.data(), n_run * sizeof(int), hipMemcpyHostToDevice, h->stream));
    for (int k = 0; k < 5; ++k)
        HIPCHK(hipMemcpyAsync(h->st_c[k], c[k].data(), n_run * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_run_out = n_run;
    h->n_run = n_run;
    h->st_valid = true; h->st_mode = mode; h->st_skip = skip; h->st_eta = eta;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// dsg_sample = prepare (x_T, step tables, control block, [AQL packet plan]) -> step loop -> finish (x_0 out).
// dsg_sample_multi runs the step loops of several handles ("lanes": own HSA queue each, shared weights) concurrently from one
// host thread.
// ---------------------------------------------------------------------------------------------------------
// How one step loop is started and run: what sample_prepare is told beside the caller's dsg_sample_args.  Built by the caller for the call
// (a window, a round) and gone with it: nothing of it is kept on the handle
struct RunMode {
    int lanes = 1;                     // the lanes that share the GPU in this call (select_kernels)
    enum { X_IN, CLIP_X_IN, CLIPQ_X_IN } start = X_IN;      // k_x_in on the call's init_noise / init_image; k_clip_x_in on window c of the handle's
    int c = 0, n_out = 0;                                    // clip-level init motion, a clip of n_out frames; k_clipq_x_in through the lane's edit table
    int inpaint = 0;                   // > 0: the pose head's epilogue reads inp32 / inp_mask, which hold a constraint for that batch
    NoiseTable noise;
};
// ... from the handle's user state: the sticky dsg_set_inpainting and dsg_set_noise_streams.  What dsg_sample / _multi run as it is and
// dsg_sample_clip starts every window from
static RunMode user_run_mode(const dsg_handle* h, int lanes) {
    RunMode m;
    m.lanes = lanes; m.inpaint = h->inpB;
    m.noise.B = h->nkB; m.noise.seeds = h->nk_seeds; m.noise.keys = h->nkeys.data();
    return m;
}

struct SampleJob {
    StepCtx c;
    int n_run = 0, B = 0, done = 0;      // n_run: steps THIS call runs; done: how many of them have been issued
    int first = 0;                       // absolute loop index of its first step (dsg_sample_args.first_step: a resumed chain)
    bool dumping = false, aql = false;
    int spg = -1;
    // what the loop did, for the call's report (run_lanes / sample_run_hip): LastRun::path, ::nofence, and with AQL packets (>= 0) the milliseconds
    int path = 0; bool nofence = false; double clock_ms = -1.0;      // on the host clock from the first doorbell to the completion signal
};
// The one writer of a handle's report (beside dsg_forward, for the kernel set alone): once per lane, where a sampling call succeeds
static void commit_report(dsg_handle* h, const SampleJob& job, int steps, double host_ms) {
    h->last = LastRun{true, steps, job.path, job.nofence, host_ms, job.c.ks.set};
}

#ifndef DSG_EMU
// One-time check of the premise of the fence-free loop on the device it is about to run on (advisor, round 2): a hand-off
// through uncached memory between two dependent AQL packets WITHOUT acquire / release must never be stale, whichever XCDs
// the writer and the reader run on.  64 x {k_uc_probe_w, k_uc_probe_r} on the handle's own queue, the same protocol as the
// step loop (device-resident iteration word, read with vector loads, advanced by an extra workgroup of the other kernel).
// A mismatch (another ASIC / ROCm version mapping hipDeviceMallocUncached differently) turns fence-free submission off for
// the process, with a warning; dsg_last_sample_fence_free then reports 0.
static std::atomic<int> g_uc_checked[64];      // per device: 0 not yet, 1 ok, 2 broken
static std::mutex g_uc_mutex;                  // one probe at a time: two host threads creating handles on one device run it once
static bool uc_selfcheck(dsg_handle* h) {
    const int dev = h->cfg.device & 63;
    if (int v = g_uc_checked[dev].load(std::memory_order_acquire)) return v == 1;
    std::lock_guard<std::mutex> lock(g_uc_mutex);
    if (int v = g_uc_checked[dev].load(std::memory_order_acquire)) return v == 1;
    const int n_wg = 256, iters = 64;
    // The 257 KB probe buffer comes from outside the pool's cap (round-5 advisor: a pool that is full at this moment is a TRANSIENT condition,
    // but the verdict stored here is permanent for the process); it goes back to the pool like every uncached block.  No uncached memory at
    // all on this device: that IS permanent.
    unsigned* buf = (unsigned*)uc_pool_take(h->cfg.device, (size_t)(n_wg * 256 + 64) * sizeof(unsigned), /*ignore_cap=*/true);
    if (!buf) {
        g_uc_checked[dev].store(2, std::memory_order_release);
        return false;
    }
    bool ok = hipMemset(buf, 0, (size_t)(n_wg * 256 + 64) * sizeof(unsigned)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    UcProbeArgs a;
    a.buf = buf; a.ctl = (int*)(buf + n_wg * 256); a.err = buf + n_wg * 256 + 16; a.n_wg = n_wg;
    const bool trace_was_armed = h->aql.trace.armed;      // (a timeline trace armed for the caller's sample is not for this run)
    h->aql.trace.armed = false;
    if (ok) {
        dsg_aql::begin(h->aql);
        ok = dsg_aql::record(h->aql, (const void*)&k_uc_probe_w, h->stream, dim3(n_wg + 1), dim3(256), &a, sizeof a) &&
             dsg_aql::record(h->aql, (const void*)&k_uc_probe_r, h->stream, dim3(n_wg + 1), dim3(256), &a, sizeof a);
        ok = dsg_aql::finish(h->aql) && ok;
        h->aql.nofence = true;
        ok = ok && dsg_aql::run(h->aql, iters, 10.0);
        h->aql.nofence = false;
    }
    h->aql.trace.armed = trace_was_armed;
    unsigned res[2] = {1u, 0u};
    if (ok) ok = hipMemcpy(res, a.err, sizeof res, hipMemcpyDeviceToHost) == hipSuccess;
    uc_pool_give(h->cfg.device, buf);      // (uncached memory goes back to the pool, never to hipFree: see UcPool)
    const bool good = ok && res[0] == 0u && res[1] == (unsigned)iters;      // no stale word seen, and the reader really ran `iters` times
    if (!good)
        fprintf(stderr, "libdsg_hip: WARNING: uncached-memory hand-off check failed on device %d (stale words: %u, iterations seen: %u of %d); "
                        "the step loop keeps its acquire / release fences\n", h->cfg.device, res[0], res[1], iters);
    g_uc_checked[dev].store(good ? 1 : 2, std::memory_order_release);
    return good;
}
#endif

#ifdef DSG_X_HOSTPROF
#include <chrono>
struct HostProf {
    double acc[16] = {0}; long n = 0; std::chrono::steady_clock::time_point t;
    void start() { t = std::chrono::steady_clock::now(); ++n; }
    void lap(int i) { auto u = std::chrono::steady_clock::now(); acc[i] += std::chrono::duration<double, std::micro>(u - t).count(); t = u; }
    ~HostProf() { if (n) { fprintf(stderr, "hostprof (us per call, %ld calls):", n); for (int i = 0; i < 16; ++i) if (acc[i] > 0) fprintf(stderr, " [%d] %.1f", i, acc[i] / n); fprintf(stderr, "\n"); } }
};
static HostProf g_hp;
#define HP_START() g_hp.start()
#define HP_LAP(i) g_hp.lap(i)
#else
#define HP_START() ((void)0)
#define HP_LAP(i) ((void)0)
#endif
// sample_prepare, piece by piece (what a piece enqueues goes on h->stream).  The refusals that need nothing but the arguments; rows: B + the twins of guidance
static int sample_check(dsg_handle* h, const dsg_sample_args* a, const RunMode& m, int B, int* rows) {
    if (!h || !a) return fail(DSG_E_INVALID, "dsg_sample: null argument");
    if (!h->finalized || !h->cond_set) return fail(DSG_E_STATE, "dsg_sample before finalize / set_window_cond");
    CHK(rows_for(h, B, rows));
    // (the user's batches: what user_run_mode took over; a window's cut and a queue's round bring the call's own B)
    if (m.inpaint > 0 && m.inpaint != B) return fail(DSG_E_INVALID, "batch differs from the batch of dsg_set_inpainting");
    if (m.noise.B > 0 && m.noise.B != B)
        return fail(DSG_E_INVALID, "batch " + std::to_string(B) + " differs from the batch of dsg_set_noise_streams (" + std::to_string(m.noise.B) + ")");
    if (a->mode != DSG_MODE_DDPM && a->mode != DSG_MODE_DDIM) return fail(DSG_E_INVALID, "mode");
    // (dump points are allowed with DDIM: ddim_sample_loop_progressive is built on them; the Python ddim_sample_loop itself
    // refuses dump_steps like the reference, gaussian_diffusion.py:913-916)
    if (a->mode == DSG_MODE_DDIM && a->const_noise)
        return fail(DSG_E_NOT_IMPLEMENTED, "ddim_sample_loop: const_noise (gaussian_diffusion.py:915-916)");
    return 0;
}
// what the start kernel of a chain reads: explicit x_T inputs on the device (null: none), the call's key, the noise block's tables (null: unkeyed)
struct StartIn { const float *noise = nullptr, *init = nullptr; NoiseKey nk; const unsigned *keys = nullptr, *offs = nullptr; };
// The noise block (GemmArgs::dyn), filled in dyn_host and uploaded in front of the start kernel, which reads its tables too (handed back in s, with the key)
static int upload_noise_block(dsg_handle* h, const dsg_sample_args* a, const NoiseTable& nt, StartIn& s) {
    unsigned *dyn = h->dyn_host.data(), *key = dyn + GemmArgs::DYN_KEY;
    set_noise_key(key, a->seed, a->stream_id);
    s.nk = NoiseKey{key[0], key[1], key[2], key[3]};
    dyn[GemmArgs::DYN_DRAW] = a->draw_base + 1u;
    const size_t pairs = GemmArgs::dyn_pairs(h->Bmax), starts = GemmArgs::dyn_starts(h->Bmax);
    for (int b = 0; b < nt.B; ++b) {
        const unsigned* k = nt.keys + 4 * (a->const_noise ? 0 : b);
        key = dyn + GemmArgs::DYN_KEYS + 4 * b;
        key[0] = nt.seeds ? k[0] : s.nk.k0; key[1] = nt.seeds ? k[1] : s.nk.k1; key[2] = k[2]; key[3] = k[3];
        dyn[pairs + 2 * b] = nt.offs ? nt.offs[b] : 0u; dyn[pairs + 2 * b + 1] = nt.holds ? (unsigned)nt.holds[b] : 0u;
        dyn[starts + b] = nt.starts ? nt.starts[b] : 0u;
    }
    const bool keyed = nt.B > 0;
    HIPCHK(hipMemcpyAsync(h->dyn, dyn, (keyed ? starts + (size_t)nt.B : GemmArgs::DYN_DRAW + 1) * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    s.keys = keyed ? h->dyn + GemmArgs::DYN_KEYS : nullptr; s.offs = keyed ? h->dyn + starts : nullptr;      // (offs: the start kernels'; GemmArgs::draw_off is the pair table)
    return 0;
}
// x_T (gaussian_diffusion.py:701-713) into the state, in the layout of the job's kernel set
static int start_chain(dsg_handle* h, const dsg_sample_args* a, const RunMode& m, const SampleJob& job, const StartIn& s) {
    const float qa = (float)h->sched.sqrt_ac[h->n_run - 1], qb = (float)h->sched.sqrt_1mac[h->n_run - 1];      // (q_sample at the chain's first timestep)
    if (m.start == RunMode::CLIPQ_X_IN)      // (a round of the clip queue on a lane that runs a job with an init motion, or of a call with per-clip skips)
        return launch_clip_x_in_q(h, s.nk, s.keys, s.offs, a->draw_base, job.B, job.c.ks);
    if (m.start == RunMode::CLIP_X_IN)       // (dsg_sample_clip on a handle with a clip-level init: it has refused init_noise / init_image / first_step)
        return launch_clip_x_in(h, m.c, m.n_out, qa, qb, s.nk, s.keys, s.offs, a->draw_base, job.B, job.c.ks);
    const int do_q = (job.first == 0 && (a->skip_timesteps > 0 || a->init_image)) ? 1 : 0;      // (a resumed chain starts from x_t as handed over)
    return launch_x_in(h, s.noise, s.init, do_q, qa, qb, s.noise ? 0 : 1, s.nk, s.keys, s.offs, a->draw_base, job.B, job.c.ks);
}
// replayed per-step noise [steps of the whole chain][n]: where it is on the device, or its upload
static int replayed_noise(dsg_handle* h, const float* step_noise, size_t n, const float** ext) {
    *ext = step_noise;
    if (!step_noise || is_device_ptr(step_noise)) return 0;
    const size_t ne = (size_t)h->n_run * n;
    if (ne > h->ext_noise_cap) { CHK(dalloc(h, &h->ext_noise, ne, false)); h->ext_noise_cap = ne; }
    HIPCHK(hipMemcpyAsync(h->ext_noise, step_noise, ne * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *ext = h->ext_noise;
    return 0;
}
#ifndef DSG_EMU
// The step loop as hand-written AQL packets (dsg_aql.h): one recording pass of run_step (no launch), argument blocks to device memory; job.aql says that
// the plan stands, and run_lanes then sends n_run x the same packets on the handle's own HSA queue.  Any failure before the first packet falls back to
// the HIP launches; a failure after submission is an error.  Not for dump points, nor where a graph is wanted
static int plan_aql(dsg_handle* h, SampleJob& job) {
    if (h->aql_mode != 1 || job.dumping || (job.spg > 0 && job.n_run >= job.spg) || job.n_run <= 0) return 0;
    bool planned = dsg_aql::init(h->aql, h->cfg.device, (const void*)&dsg_version);
    const bool nofence = planned && h->uc_mode == 1 && uc_selfcheck(h);
    HP_LAP(3);
    if (planned) {
        dsg_aql::begin(h->aql);
        const int rc = run_step_p(h, job.c);
        HP_LAP(4);
        planned = dsg_aql::finish(h->aql) && rc == 0;
        HP_LAP(5);
        h->aql.recording = false;
        h->aql.nofence = nofence;            // fence-free packets (see uc_mode; 2: uncached buffers behind the usual fences)
    }
    if (!planned) {
        if (!h->aql_warned) { fprintf(stderr, "libdsg_hip: AQL path unavailable (%s); using HIP launches\n", h->aql.err.c_str()); h->aql_warned = true; }
        h->aql_mode = 0;
        return 0;
    }
    HIPCHK(hipStreamSynchronize(h->stream));         // state / control block / conditioning are in place
    job.aql = true;
    return 0;
}
#endif

static int sample_prepare(dsg_handle* h, const dsg_sample_args* a, const RunMode& m, int B, void* stream, SampleJob& job) {
    int rows = 0;
    CHK(sample_check(h, a, m, B, &rows));
    HIPCHK(hipSetDevice(h->cfg.device));
    HP_START();
    CHK(order_after(h, stream));
    int n_total = 0;
    CHK(build_step_tables(h, a->mode, a->skip_timesteps, a->eta, &n_total));
    HP_LAP(0);
    // a chain may be run in pieces (first_step / max_steps: the lazy generator forms of the loops): steps [first, first + n_run)
    const int first = a->first_step;
    if (first < 0 || first >= n_total || a->max_steps < 0) return fail(DSG_E_INVALID, "first_step / max_steps out of range");
    if (first > 0 && !a->init_noise) return fail(DSG_E_INVALID, "first_step > 0 resumes a chain: init_noise must hold x_t of that step");
    job = SampleJob();      // (a caller's job serves window after window); n_run: the steps of this call (the tables keep the whole chain: h->n_run)
    job.B = B; job.first = first; job.n_run = a->max_steps > 0 ? std::min(a->max_steps, n_total - first) : n_total - first;
    const size_t n = (size_t)B * h->J * h->T;
    StartIn s;
    CHK(to_dev(h, a->init_noise, h->io_tmp, n, &s.noise));
    CHK(to_dev(h, a->init_image, h->io_tmp2, n, &s.init));
    StepCtx& c = job.c;
    CHK(select_kernels(h, rows, m.lanes, c.ks));      // (first: the layout of the state shadow belongs to the kernel set)
    CHK(ensure_set_buffers(h, c.ks));
    CHK(upload_noise_block(h, a, m.noise, s));
    CHK(start_chain(h, a, m, job, s));
    CHK(replayed_noise(h, a->step_noise, n, &c.ext_noise));
    hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(64), 0, h->stream, h->ctl, h->st_tmodel, first);
    HIPCHK(hipGetLastError());
    HP_LAP(1);
    HIPCHK(hipStreamSynchronize(h->stream));      // (the upload of `dyn` above has landed)
    HP_LAP(2);
    c.B = rows; c.out_mode = a->mode == DSG_MODE_DDPM ? OUT_DDPM : OUT_DDIM; c.use_ctr = true;
    c.const_noise = a->const_noise; c.keyed = m.noise.B > 0 ? 1 : 0; c.clip_x0 = a->clip_denoised ? 1 : 0;
    c.no_noise = (a->mode == DSG_MODE_DDIM && a->eta == 0.f && !c.ext_noise) ? 1 : 0;
    c.inpaint = m.inpaint > 0 ? 1 : 0;     // (the AQL argument blocks are recorded anew below for every call: on / off needs no invalidation)
    job.dumping = a->n_dump > 0 && a->dump_steps && a->dump_out;
    // steps_per_graph: 0 = default = no hipGraph.  Measured on MI355X / ROCm 7.2: hipGraph replay of the step is slower than
    // stream-ordered HIP launches (180 vs 157 us; 151-163 us with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0), and both lose to the
    // hand-written AQL submission (139 us) -- graphs stay opt-in (steps_per_graph > 0).
    job.spg = h->cfg.steps_per_graph == 0 ? -1 : h->cfg.steps_per_graph;
    if (job.dumping || c.ext_noise) job.spg = -1;           // rare paths run eagerly (ext pointer / dump points are per call)
#ifndef DSG_EMU
    CHK(plan_aql(h, job));
#endif
    HIPCHK(hipEventRecord(h->ev_t0, h->stream));
    HP_LAP(6);
    return 0;
}

// the step loop through the HIP runtime: hipGraph replays (opt-in) and / or stream-ordered launches
static int sample_run_hip(dsg_handle* h, const dsg_sample_args* a, SampleJob& job) {
    const int n_run = job.n_run, B = job.B, spg = job.spg;
    const StepCtx& c = job.c;
    const size_t n = (size_t)B * h->J * h->T;
    if (spg > 0 && n_run >= spg && job.done == 0) {
        // everything that varies between calls (step index, coefficients, noise key, conditioning) lives in device
        // memory, so one captured graph per (batch, sampler, mask batch, const_noise, steps, flags, kernel set) serves every window and clip
        dsg_handle::GKey key = {c.B, c.out_mode, h->mb, c.const_noise, n_run, h->n_run, (c.clip_x0 ? 1 : 0) | (h->cfgB ? 2 : 0) | (h->nomask ? 4 : 0) | (c.ks.attn_in_mid ? 8 : 0) | (c.no_noise ? 16 : 0) | (c.inpaint ? 32 : 0) | (c.keyed ? 64 : 0),
                                c.ks.set};
        auto it = h->graphs.find(key);
        bool ok = true;
        if (it == h->graphs.end()) {
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                int rc = 0;
                for (int s = 0; s < spg && rc == 0; ++s) rc = run_step_p(h, c);
                e = hipStreamEndCapture(h->stream, &graph);
                if (rc != 0 || e != hipSuccess || !graph) ok = false;
                if (ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) ok = false;
            } else ok = false;
            if (!ok) { (void)hipGetLastError(); if (graph) (void)hipGraphDestroy(graph); }
            else {
                dsg_handle::GVal v = {exec, graph, spg};
                it = h->graphs.emplace(key, v).first;
            }
        }
        if (ok) {
            while (n_run - job.done >= spg) { HIPCHK(hipGraphLaunch(it->second.exec, h->stream)); job.done += spg; }
            job.path = 2;      // (also when trailing steps follow eagerly below)
        }
    }
    int di = 0;
    for (; job.done < n_run; ++job.done) {
        CHK(run_step_p(h, c));
        if (job.dumping) {
            while (di < a->n_dump && a->dump_steps[di] < job.first + job.done) ++di;
            if (di < a->n_dump && a->dump_steps[di] == job.first + job.done) {
                CHK(launch_x_out(h, h->fwd_out, B));
                CHK(from_dev(h, a->dump_out + (size_t)di * n, h->fwd_out, n));
                ++di;
            }
        }
    }
    return 0;
}

// The step loops of n prepared lanes, run to their end: one lane as dsg_sample always ran it (its own AQL queue, or HIP launches / graph
// replays), several interleaved (AQL: one queue per lane, the steps dealt round-robin by this host thread; HIP launches: step s of every
// lane, then s + 1).  Shared by dsg_sample, dsg_sample_multi and the windows of dsg_sample_clip.
static int run_lanes(dsg_handle** hs, int n, const dsg_sample_args* args, SampleJob* jobs) {
    if (n == 1) {
        dsg_handle* h = hs[0];
        SampleJob& job = jobs[0];
#ifndef DSG_EMU
        if (job.aql) {
            if (!dsg_aql::run(h->aql, job.n_run, 60.0 + 0.01 * job.n_run)) return fail(DSG_E_RUNTIME, "AQL run: " + h->aql.err);
            job.done = job.n_run;
            job.path = 1; job.nofence = h->aql.nofence; job.clock_ms = h->aql.run_ms;
        }
#endif
        return sample_run_hip(h, &args[0], job);
    }
    bool all_aql = true;
    for (int i = 0; i < n; ++i) all_aql = all_aql && jobs[i].aql;
#ifndef DSG_EMU
    if (all_aql) {
        std::vector<dsg_aql::Ctx*> ctxs(n);
        std::vector<int> steps(n);
        double tmax = 60.0;
        for (int i = 0; i < n; ++i) { ctxs[i] = &hs[i]->aql; steps[i] = jobs[i].n_run; tmax += 0.01 * jobs[i].n_run; }
        std::string err;
        if (!dsg_aql::run_multi(ctxs.data(), steps.data(), n, tmax, err)) return fail(DSG_E_RUNTIME, "AQL run: " + err);
        for (int i = 0; i < n; ++i) {
            jobs[i].done = jobs[i].n_run;
            jobs[i].path = 1; jobs[i].nofence = hs[i]->aql.nofence; jobs[i].clock_ms = hs[i]->aql.run_ms;
        }
    }
#endif
    if (!all_aql) {
        // HIP launches: an AQL plan that was recorded for some lanes is simply not used; step s of every lane, then s + 1
        bool plain = true;
        for (int i = 0; i < n; ++i) plain = plain && !jobs[i].dumping && !(jobs[i].spg > 0 && jobs[i].n_run >= jobs[i].spg);
        if (plain) {
            int more = 1;
            for (int s = 0; more; ++s) {
                more = 0;
                for (int i = 0; i < n; ++i)
                    if (s < jobs[i].n_run) { CHK(run_step_p(hs[i], jobs[i].c)); jobs[i].done = s + 1; more = 1; }
            }
        }
    }
    for (int i = 0; i < n; ++i) CHK(sample_run_hip(hs[i], &args[i], jobs[i]));      // whatever is left (graphs, dump points); nothing after AQL
    return 0;
}

static int sample_finish(dsg_handle* h, float* out, void* stream, SampleJob& job) {
    const size_t n = (size_t)job.B * h->J * h->T;
    HP_LAP(7);                               // (the step loop itself)
    HIPCHK(hipEventRecord(h->ev_t1, h->stream));
    commit_report(h, job, job.n_run, job.clock_ms);      // (not timed by the AQL clock: the two events, resolved when asked)
    CHK(launch_x_out(h, h->fwd_out, job.B));
    CHK(from_dev(h, out, h->fwd_out, n));
    CHK(order_before(h, stream));
    HP_LAP(8);
    return 0;
}

extern "C" int dsg_sample(dsg_handle* h, const dsg_sample_args* a, float* out, int B, void* stream) {
    if (!h || !a || !out) return fail(DSG_E_INVALID, "dsg_sample: null argument");
    CHK(owned_by_queue(h));
    SampleJob job;
    CHK(sample_prepare(h, a, user_run_mode(h, 1), B, stream, job));
    CHK(run_lanes(&h, 1, a, &job));
    return sample_finish(h, out, stream, job);
}

// n lanes (handles of ONE device, normally a handle and its clones), one independent sampling call each, advanced
// concurrently.  With the AQL submission every lane has its own HSA queue and the host thread deals the steps round-robin (the
// queues' dependent packet chains overlap on the GPU); with HIP launches the lanes' streams are fed step by step.  Every lane
// runs the kernel set ITS handle selects (dsg_set_kernel_set / the batch): the call changes nothing about the arithmetic, so
// lane i's sample is bit-identical to dsg_sample(lanes[i], &args[i], ...) on its own.
extern "C" int dsg_sample_multi(dsg_handle** hs, int n, const dsg_sample_args* args, float** outs, int B, void* stream) {
    if (!hs || !args || !outs || n <= 0) return fail(DSG_E_INVALID, "dsg_sample_multi: bad argument");
    for (int i = 0; i < n; ++i) {
        if (!hs[i] || !outs[i]) return fail(DSG_E_INVALID, "dsg_sample_multi: null handle / output");
        CHK(owned_by_queue(hs[i]));
        for (int j = 0; j < i; ++j) if (hs[j] == hs[i]) return fail(DSG_E_INVALID, "dsg_sample_multi: a handle appears twice");
        if (hs[i]->cfg.device != hs[0]->cfg.device) return fail(DSG_E_INVALID, "dsg_sample_multi: lanes must live on one device");
    }
    if (n > 16) return fail(DSG_E_INVALID, "dsg_sample_multi: at most 16 lanes (4 overlap on the hardware; put further clips into the lanes' batches)");
    std::vector<SampleJob> jobs(n);
    for (int i = 0; i < n; ++i) CHK(sample_prepare(hs[i], &args[i], user_run_mode(hs[i], n), B, stream, jobs[i]));
    CHK(run_lanes(hs, n, args, jobs.data()));
    for (int i = 0; i < n; ++i) CHK(sample_finish(hs[i], outs[i], stream, jobs[i]));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// dsg_sample_clip / dsg_sample_clip_multi: all K windows of the B clips of every lane in one call -- the window loops of
// main/mydiffusion_zeggs/sample.py:236-296 and BEAT-TWH-main/mydiffusion_beat_twh/sample.py:98-192.  Per window: the conditioning
// (set_window_cond, y['seed'] = the tail the previous hand-off left in c_seed), sample_prepare + the step loop exactly as dsg_sample
// / dsg_sample_multi issue them, then k_window_handoff in place of k_x_out + the copy to the caller.  One copy of the stitched clip
// at the end.  Bit-identical to the K calls + the host stitching of sample.py: the same kernels, draws and fp32 operations.
// ---------------------------------------------------------------------------------------------------------
static int launch_handoff(dsg_handle* h, float* clip_out, int B, int n_out, int c, int K, int root_shift, int keep_last_tail) {
    HandoffArgs a;
    a.xs32 = h->xs32; a.tail_in = h->clip_tail[(c + 1) & 1]; a.tail_out = h->clip_tail[c & 1]; a.c_seed = h->c_seed; a.clip_out = clip_out;
    a.B = B; a.J = h->J; a.Jp = h->Jp; a.T = h->T; a.S = h->S; a.n_out = n_out; a.c = c;
    a.root_shift = root_shift ? 1 : 0; a.is_first = c == 0 ? 1 : 0; a.is_last = c == K - 1 ? 1 : 0; a.keep_last_tail = keep_last_tail ? 1 : 0;
    return launch_state(h, k_window_handoff, B, a);
}

static int launch_clip_inp_window(dsg_handle* h, int B, int n_out, int c) {
    ClipInpArgs a;
    a.motion = h->cinp_motion; a.mask = h->cinp_mask; a.inp32 = h->inp32; a.inp_mask = h->inp_mask;
    a.B = B; a.J = h->J; a.Jp = h->Jp; a.T = h->T; a.S = h->S; a.n_out = n_out; a.c = c;
    return launch_state(h, k_clip_inp_window, B, a);
}

// the two copies of the hand-off's tail, on first use: for the window loop below and for the rounds of a queue
static int clip_tails_ready(dsg_handle* h) {
    for (int k = 0; k < 2; ++k)
        if (!h->clip_tail[k]) CHK(dalloc(h, &h->clip_tail[k], (size_t)h->Bmax * h->J * h->S));
    return 0;
}
// The step loop of a window (of a queue's round) has been issued on lane h: its time -- the AQL run's host clock, else the events around the
// loop, waited for here -- goes onto `sum`, the caller's, which is what dsg_last_sample_ms reports for the call.  The hand-off follows
static int clip_window_timed(dsg_handle* h, const SampleJob& job, double& sum) {
    HIPCHK(hipEventRecord(h->ev_t1, h->stream));
    if (job.clock_ms >= 0.0) { sum += job.clock_ms; return 0; }
    float ms = 0.f;
    HIPCHK(hipEventSynchronize(h->ev_t1));
    HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
    sum += ms;
    return 0;
}

static int sample_clip(dsg_handle** hs, int n, const float* const* styles, const float* const* seed0s, const float* const* audios,
                       const uint8_t* mask_local, int mask_batch, const float* const* scales, const dsg_sample_args* args, int K,
                       int root_shift, int keep_last_tail, float** outs, int B, void* stream) {
    if (!hs || !styles || !audios || !args || !outs || n <= 0) return fail(DSG_E_INVALID, "dsg_sample_clip: bad argument");
    if (n > 16) return fail(DSG_E_INVALID, "dsg_sample_clip_multi: at most 16 lanes (4 overlap on the hardware; put further clips into the lanes' batches)");
    if (K < 1) return fail(DSG_E_INVALID, "dsg_sample_clip: K < 1");
    for (int i = 0; i < n; ++i) {
        dsg_handle* h = hs[i];
        if (!h || !outs[i] || !styles[i] || !audios[i]) return fail(DSG_E_INVALID, "dsg_sample_clip: null handle / style / audio / output");
        CHK(owned_by_queue(h));
        for (int j = 0; j < i; ++j) if (hs[j] == h) return fail(DSG_E_INVALID, "dsg_sample_clip_multi: a handle appears twice");
        if (h->cfg.device != hs[0]->cfg.device) return fail(DSG_E_INVALID, "dsg_sample_clip_multi: lanes must live on one device");
        if (h->J != hs[0]->J || h->T != hs[0]->T || h->S != hs[0]->S) return fail(DSG_E_INVALID, "dsg_sample_clip_multi: lanes of one model");
        if (!h->finalized) return fail(DSG_E_STATE, "dsg_sample_clip before dsg_finalize_weights");
        if (h->sched.n == 0) return fail(DSG_E_STATE, "dsg_sample_clip before dsg_set_schedule");
        if (h->S <= 0 || 2 * h->S >= h->T) return fail(DSG_E_INVALID, "dsg_sample_clip: the window hand-off needs 0 < 2 * n_seed < n_poses");
        if (h->inpB > 0) return fail(DSG_E_INVALID, "dsg_sample_clip: an inpainting constraint is per window (dsg_set_inpainting(h, NULL, NULL, ...) first)");
        const dsg_sample_args& a = args[i];
        if (a.step_noise || a.n_dump || a.first_step || a.max_steps || a.init_noise || a.init_image)
            return fail(DSG_E_INVALID, "dsg_sample_clip: step_noise / dump_steps / first_step / max_steps / init_noise / init_image are per window");
        if (a.skip_timesteps < 0 || a.skip_timesteps >= h->sched.n) return fail(DSG_E_INVALID, "skip_timesteps out of range");
        if (a.skip_timesteps != args[0].skip_timesteps || h->sched.n != hs[0]->sched.n) return fail(DSG_E_INVALID, "dsg_sample_clip_multi: one step count for every lane");
        const int rows = (scales && scales[i]) ? 2 * B : B;
        if (B <= 0 || rows > h->Bmax) return fail(DSG_E_INVALID, rows > B ? "classifier-free guidance needs max_batch >= 2 * batch" : "batch exceeds max_batch");
    }
    const int T = hs[0]->T, S = hs[0]->S, J = hs[0]->J;
    const int n_out = keep_last_tail ? K * (T - S) : K * (T - S) - S;
    const size_t n_clip = (size_t)B * n_out * J, n_tail = (size_t)B * J * S;
    const int n_run = hs[0]->sched.n - args[0].skip_timesteps;
    for (int i = 0; i < n; ++i) {          // a clip-level constraint (dsg_set_clip_inpainting) is in the coordinates of THIS call's `out`
        const dsg_handle* h = hs[i];
        if (h->cinpB > 0 && h->cinpB != B)
            return fail(DSG_E_INVALID, "dsg_sample_clip: batch " + std::to_string(B) + " differs from the batch of dsg_set_clip_inpainting (" + std::to_string(h->cinpB) + ")");
        if (h->cinpB > 0 && h->cinp_frames != n_out)
            return fail(DSG_E_INVALID, "dsg_sample_clip: the clip has n_out = " + std::to_string(n_out) + " frames, the constraint of dsg_set_clip_inpainting n_frames = " +
                                       std::to_string(h->cinp_frames));
        if (h->cinitB > 0 && h->cinitB != B)
            return fail(DSG_E_INVALID, "dsg_sample_clip: batch " + std::to_string(B) + " differs from the batch of dsg_set_clip_init (" + std::to_string(h->cinitB) + ")");
        if (h->cinitB > 0 && h->cinit_frames != n_out)
            return fail(DSG_E_INVALID, "dsg_sample_clip: the clip has n_out = " + std::to_string(n_out) + " frames, the init motion of dsg_set_clip_init n_frames = " +
                                       std::to_string(h->cinit_frames));
    }
    HIPCHK(hipSetDevice(hs[0]->cfg.device));
    std::vector<float*> clip(n);
    for (int i = 0; i < n; ++i) {
        dsg_handle* h = hs[i];
        CHK(clip_tails_ready(h));
        if (is_device_ptr(outs[i])) clip[i] = outs[i];      // the hand-off writes the caller's tensor itself
        else {
            if (n_clip > h->clip_out_cap) { CHK(dalloc(h, &h->clip_out, n_clip, false)); h->clip_out_cap = n_clip; }
            clip[i] = h->clip_out;
        }
        // y['seed'] of window 0: the caller's, or zeros (sample.py:241) -- in place, where the hand-off leaves the later ones
        CHK(order_after(h, stream));
        if (seed0s && seed0s[i]) CHK(upload(h, h->c_seed, seed0s[i], n_tail * sizeof(float)));
        else HIPCHK(hipMemsetAsync(h->c_seed, 0, n_tail * sizeof(float), h->stream));
    }
    std::vector<SampleJob> jobs(n);
    std::vector<double> ms(n, 0.0);      // per lane: the sum over its windows
    std::vector<dsg_sample_args> wargs(args, args + n);
    // Every window runs as dsg_sample_multi would run it on the lane's user state (the noise streams; inpB == 0, checked above), but for:
    // Lanes with a clip-level constraint: window c's slice goes into inp32 / inp_mask where the window's conditioning is set -- on the handle's
    // stream, which sample_prepare drains before the first packet, whose acquire covers it like the conditioning; the pointers stay, only the
    // contents change -- and the epilogue's inpainting is on (StepCtx::inpaint, GKey flag 32).
    // Lanes with a clip-level init motion: sample_prepare starts window c from q_sample of its slice (k_clip_x_in reads c_seed for the frames in
    // front of the clip: window 0's y['seed'], uploaded above on the same stream)
    std::vector<RunMode> modes(n);
    for (int i = 0; i < n; ++i) {
        modes[i] = user_run_mode(hs[i], n);
        if (hs[i]->cinpB > 0) modes[i].inpaint = B;
        if (hs[i]->cinitB > 0) { modes[i].start = RunMode::CLIP_X_IN; modes[i].n_out = n_out; }
    }
    for (int c = 0; c < K; ++c) {
        for (int i = 0; i < n; ++i) {
            dsg_handle* h = hs[i];
            const float* audio_c = audios[i] + (size_t)c * B * h->Ta * h->As;
            CHK(set_window_cond(h, styles[i], h->c_seed, audio_c, mask_local, mask_batch, B, 0, scales ? scales[i] : nullptr, stream));
            if (h->cinpB > 0) CHK(launch_clip_inp_window(h, B, n_out, c));
            modes[i].c = c;
            wargs[i].draw_base = args[i].draw_base + (uint32_t)c * (uint32_t)(1 + n_run);      // what K consecutive dsg_sample calls consume
        }
        for (int i = 0; i < n; ++i) CHK(sample_prepare(hs[i], &wargs[i], modes[i], B, stream, jobs[i]));
        CHK(run_lanes(hs, n, wargs.data(), jobs.data()));
        for (int i = 0; i < n; ++i) {
            CHK(clip_window_timed(hs[i], jobs[i], ms[i]));
            CHK(launch_handoff(hs[i], clip[i], B, n_out, c, K, root_shift, keep_last_tail));
        }
    }
    for (int i = 0; i < n; ++i) {
        dsg_handle* h = hs[i];
        commit_report(h, jobs[i], K * n_run, ms[i]);
        if (clip[i] != outs[i]) CHK(from_dev(h, outs[i], clip[i], n_clip));
        CHK(order_before(h, stream));
    }
    return 0;
}
extern "C" int dsg_sample_clip(dsg_handle* h, const float* style, const float* seed0, const float* audio, const uint8_t* mask_local,
                               int mask_batch, const float* scale, const dsg_sample_args* args, int K, int root_shift,
                               int keep_last_tail, float* out, int B, void* stream) {
    return sample_clip(&h, 1, &style, &seed0, &audio, mask_local, mask_batch, &scale, args, K, root_shift, keep_last_tail, &out, B, stream);
}
extern "C" int dsg_sample_clip_multi(dsg_handle** lanes, int n, const float* const* styles, const float* const* seed0s,
                                     const float* const* audios, const uint8_t* mask_local, int mask_batch, const float* const* scales,
                                     const dsg_sample_args* args, int K, int root_shift, int keep_last_tail, float** outs, int B,
                                     void* stream) {
    return sample_clip(lanes, n, styles, seed0s, audios, mask_local, mask_batch, scales, args, K, root_shift, keep_last_tail, outs, B, stream);
}

// ---------------------------------------------------------------------------------------------------------
// The clip queue: clips of different lengths over one batch of slots, in rounds.  The round is written once (QueueRound, below); the
// one-shot call (dsg_sample_clip_queue_steps and the two exports in front of it: all jobs known, placed by a plan) and the session
// (dsg_queue_*: jobs arrive while it runs) each say what the slots run and how the jobs' tensors reach the lanes.
// ---------------------------------------------------------------------------------------------------------
// The placement, written once for both exports: jobs in the order n_run descending (where given), K descending, index ascending; each to the
// slot with the fewest rounds so far, ties to the lowest slot.  `who`: the export's name, for the messages
static int clip_queue_place(const char* who, const int32_t* K, const int32_t* n_run, int n_jobs, int n_slots, int32_t* slot, int32_t* first_round,
                            int32_t* n_rounds) {
    const std::string w(who);
    if (!K || !slot || !first_round || !n_rounds) return fail(DSG_E_INVALID, w + ": null argument");
    if (n_jobs < 1) return fail(DSG_E_INVALID, w + ": n_jobs < 1");
    if (n_slots < 1) return fail(DSG_E_INVALID, w + ": n_slots < 1");
    for (int j = 0; j < n_jobs; ++j) {
        if (K[j] < 1) return fail(DSG_E_INVALID, w + ": job " + std::to_string(j) + " has K < 1");
        if (n_run && n_run[j] < 1) return fail(DSG_E_INVALID, w + ": job " + std::to_string(j) + " has n_run < 1");
    }
    std::vector<int> order(n_jobs);
    for (int j = 0; j < n_jobs; ++j) order[j] = j;
    // deepest first, then longest, ties by lower index
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_run && n_run[a] != n_run[b] ? n_run[a] > n_run[b] : K[a] > K[b]; });
    std::vector<int64_t> load(n_slots, 0);
    int64_t most = 0;
    for (int j : order) {
        int best = 0;
        for (int s = 1; s < n_slots; ++s) if (load[s] < load[best]) best = s;      // fewest rounds so far, ties: lowest slot
        if (load[best] + K[j] > 0x7fffffff) return fail(DSG_E_INVALID, w + ": more than 2^31 - 1 rounds");
        slot[j] = best; first_round[j] = (int32_t)load[best];
        load[best] += K[j];
        most = std::max(most, load[best]);
    }
    *n_rounds = (int32_t)most;
    return 0;
}
extern "C" int dsg_clip_queue_plan(const int32_t* K, int n_jobs, int n_slots, int32_t* slot, int32_t* first_round, int32_t* n_rounds) {
    return clip_queue_place("dsg_clip_queue_plan", K, nullptr, n_jobs, n_slots, slot, first_round, n_rounds);
}
// The plan with a step count per job (dsg_sample_clip_queue_steps: n_run[j] = schedule length - the job's skip_timesteps): the deep jobs go
// first, so the closing rounds hold only light ones and run short.  A round is as long as the deepest job alive in it.  n_run == NULL (all
// equal): the order and outputs of dsg_clip_queue_plan
extern "C" int dsg_clip_queue_plan_steps(const int32_t* K, const int32_t* n_run, int n_jobs, int n_slots, int32_t* slot, int32_t* first_round,
                                         int32_t* n_rounds, int64_t* total_steps) {
    CHK(clip_queue_place("dsg_clip_queue_plan_steps", K, n_run, n_jobs, n_slots, slot, first_round, n_rounds));
    if (total_steps) {
        if (!n_run) *total_steps = *n_rounds;
        else {
            // the deepest job alive per round: a job covers rounds [first, first + K) -- swept by the rounds at which jobs begin and end
            std::vector<std::pair<int64_t, int>> ev;      // (round, +-n_run): an end sorts in front of a begin of the same round
            ev.reserve(2 * (size_t)n_jobs);
            for (int j = 0; j < n_jobs; ++j) { ev.emplace_back(first_round[j], n_run[j]); ev.emplace_back((int64_t)first_round[j] + K[j], -n_run[j]); }
            std::sort(ev.begin(), ev.end());
            std::multiset<int> alive;
            int64_t total = 0, at = 0;
            for (const auto& e : ev) {
                if (e.first > at) { if (!alive.empty()) total += (e.first - at) * (int64_t)*alive.rbegin(); at = e.first; }
                if (e.second > 0) alive.insert(e.second); else alive.erase(alive.find(-e.second));
            }
            *total_steps = total;
        }
    }
    return 0;
}

static int launch_clip_inp_window_q(dsg_handle* h, int B) {
    ClipInpQArgs a;
    a.slots = h->cq.edits; a.inp32 = h->inp32; a.inp_mask = h->inp_mask;
    a.B = B; a.J = h->J; a.Jp = h->Jp; a.T = h->T; a.S = h->S;
    return launch_state(h, k_clipq_inp_window, B, a);
}
static int launch_handoff_q(dsg_handle* h, int B, int root_shift, int keep_last_tail) {
    HandoffQArgs a;      // (which tail a slot reads and which it writes: per slot, by its window index -- in the kernel)
    a.xs32 = h->xs32; a.tail0 = h->clip_tail[0]; a.tail1 = h->clip_tail[1]; a.c_seed = h->c_seed; a.slots = h->cq.slots;
    a.B = B; a.J = h->J; a.Jp = h->Jp; a.T = h->T; a.S = h->S;
    a.root_shift = root_shift ? 1 : 0; a.keep_last_tail = keep_last_tail ? 1 : 0;
    return launch_state(h, k_window_handoff_q, B, a);
}

// The checks of a queue on its lanes, B, guided and args, and on one job: written once for dsg_sample_clip_queue_steps and the session
// (dsg_queue_open / dsg_queue_submit), which make the same refusals with the same messages.  A lane that carries noise streams or a
// constraint (and dsg_sample_clip's lane with inpB > 0) is refused as a matter of the API -- the call would have to say which of the two
// wins -- not for safety: a round's RunMode neither reads nor writes that state
static int clip_queue_check_lanes(dsg_handle** hs, int n, int B, int guided, const dsg_sample_args* args) {
    for (int i = 0; i < n; ++i) {
        dsg_handle* h = hs[i];
        if (!h) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: null handle");
        CHK(owned_by_queue(h));
        for (int j = 0; j < i; ++j) if (hs[j] == h) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: a handle appears twice");
        if (!h->finalized) return fail(DSG_E_STATE, "dsg_sample_clip_queue before dsg_finalize_weights");
        if (h->sched.n == 0) return fail(DSG_E_STATE, "dsg_sample_clip_queue before dsg_set_schedule");
        if (h->cfg.device != hs[0]->cfg.device) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: lanes must live on one device");
        if (h->J != hs[0]->J || h->T != hs[0]->T || h->S != hs[0]->S || h->Ta != hs[0]->Ta || h->As != hs[0]->As ||
            h->cfg.style_dim_in != hs[0]->cfg.style_dim_in || h->cfg.variant != hs[0]->cfg.variant)
            return fail(DSG_E_INVALID, "dsg_sample_clip_queue: lanes of one model");
        if (h->sched.n != hs[0]->sched.n) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: one step count for every lane");
        if (h->S <= 0 || 2 * h->S >= h->T) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: the window hand-off needs 0 < 2 * n_seed < n_poses");
        const int rows = guided ? 2 * B : B;
        if (B < 1) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: B < 1");
        if (rows > h->Bmax) return fail(DSG_E_INVALID, guided ? "dsg_sample_clip_queue: classifier-free guidance needs max_batch >= 2 * B" : "dsg_sample_clip_queue: B exceeds max_batch");
        if (h->nkB > 0) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: the handle carries noise streams (dsg_set_noise_streams(h, NULL, NULL, 0) first): every job brings its own pair");
        if (h->inpB > 0) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: the handle carries a window-level inpainting constraint (dsg_set_inpainting(h, NULL, NULL, ...) first)");
        if (h->cinpB > 0) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: the handle carries a clip-level inpainting constraint (dsg_set_clip_inpainting(h, NULL, NULL, ...) first): a queue takes per-clip inpainting per job (dsg_sample_clip_queue_edit)");
        if (h->cinitB > 0) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: the handle carries a clip-level init motion (dsg_set_clip_init(h, NULL, ...) first): a queue takes per-clip init motion per job (dsg_sample_clip_queue_edit)");
    }
    if (args->step_noise || args->init_noise || args->init_image || args->n_dump || args->first_step || args->max_steps || args->const_noise)
        return fail(DSG_E_INVALID, "dsg_sample_clip_queue: step_noise / init_noise / init_image / dump_steps / first_step / max_steps / const_noise are not for a queue of clips");
    if (args->mode != DSG_MODE_DDPM && args->mode != DSG_MODE_DDIM) return fail(DSG_E_INVALID, "mode");
    return 0;
}
static int clip_queue_check_job(const dsg_clip_job& q, const dsg_clip_edit* edit, int64_t j, int variant5, bool no_audio_yet = false) {
    if (q.K < 1) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: job " + std::to_string(j) + " has K < 1");
    if (!q.style || (!q.audio && !no_audio_yet) || !q.out) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: job " + std::to_string(j) + " has a null style / audio / out");
    if (variant5 && !q.seed_last) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: variant 5 needs seed_last for every job (job " + std::to_string(j) + " has none)");
    if (edit && !edit->inp_mask != !edit->inp_motion)
        return fail(DSG_E_INVALID, "dsg_sample_clip_queue_edit: inp_mask and inp_motion go together (both NULL: no constraint); job " + std::to_string(j) + " has one of them");
    return 0;
}

// What a slot runs in a round: one window of one clip.  A dead slot is the absence of one -- a null pointer in the round's table
struct SlotWork {
    dsg_clip_job job;           // the job, its pointers as they are read: the caller's (host or device), or a session's device copies
    EditSlot ed;                // motion / mask / init as the device reads them and n_out; QueueRound fills in c and the chain's start
    float* clip = nullptr;      // [ed.n_out][J] on the device: where the hand-off writes
    int c = 0;                  // the window the slot stands on
    int skip = 0, n_run = 0;    // the job's skip_timesteps and the steps of one of its windows (schedule length - skip)
    const float* win_audio = nullptr;      // a live job of a session: the audio of window c, where it is read (null: job.audio + c * n_audio)
    const float* resume = nullptr;         // a session's job that takes a slot again on window c > 0: the parked [S][J] tail, for this round only
};

// The lane's device buffers for the rounds of a queue, on first use
enum { QL_EDITS = 1, QL_GATHER = 2, QL_INP = 4 };      // + the edit table, + the gather table, + the epilogue's inpainting buffers
static int queue_lane_ready(dsg_handle* h, int flags) {
    dsg_handle::Queue& q = h->cq;
    CHK(clip_tails_ready(h));
    if (!q.style) CHK(dalloc(h, &q.style, (size_t)h->Bmax * h->cfg.style_dim_in));
    if (!q.audio) CHK(dalloc(h, &q.audio, (size_t)h->Bmax * h->Ta * h->As));
    if (!q.slots) CHK(dalloc(h, &q.slots, (size_t)h->Bmax));
    if ((flags & QL_EDITS) && !q.edits) CHK(dalloc(h, &q.edits, (size_t)h->Bmax));
    if ((flags & QL_GATHER) && !q.gather) CHK(dalloc(h, &q.gather, (size_t)h->Bmax));
    if (flags & QL_INP) {      // (each pointer on its own, as dsg_set_inpainting)
        if (!h->inp32) CHK(dalloc(h, &h->inp32, (size_t)h->Bmax * h->T * h->Jp));
        if (!h->inp_mask) CHK(dalloc(h, &h->inp_mask, (size_t)h->Bmax * h->T * h->Jp));
    }
    return 0;
}

// A job's tensor as the device reads it: where it is when that is device memory (or null), else its copy, made on h's stream, in the
// `bytes` that room(bytes, &p) hands out -- a piece of the lane's staging (the one-shot call) or a block of the session's
template <class Room>
static int staged(dsg_handle* h, const void* src, size_t bytes, Room&& room, const void** dst) {
    if (!src || is_device_ptr(src)) { *dst = src; return 0; }
    void* p = nullptr;
    CHK(room(bytes, &p));
    HIPCHK(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, h->stream));
    *dst = p;
    return 0;
}

// One round of a clip queue, for every lane: one iteration of sample_clip's window loop at the constant batch B, with per-slot
// conditioning, Philox keys, draw offsets and hand-off.  Written once, under dsg_sample_clip_queue_steps and the session (dsg_queue_run);
// the callers decide what every slot runs (`slots`), how a lane's conditioning reaches it (`cond`) and which lanes go through the edit
// table (`lane_inp`, `lane_init`).  Per lane, in stream order: the hand-off table, the conditioning (cond, set_window_cond), the edit table
// and the round's constraint (k_clipq_inp_window); then sample_prepare for every lane, the step loops (run_lanes), and per lane the timing
// and the hand-off (k_window_handoff_q).  The tables go up behind the previous round's hand-off on the lane's stream and in front of the
// point where sample_prepare drains it: their host copies are free to change in the next round.
// Round r runs from s_r = the smallest skip alive in it, over all lanes, as dsg_sample does with skip_timesteps = s_r; a slot with a larger
// skip holds for skip - s_r loop indices (DrawOff::hold).  A slot on window c of its clip draws what dsg_sample_clip draws for window c of
// that clip alone.  A dead slot runs on whatever conditioning it holds -- rows are independent -- and writes nothing
struct QueueRound {
    std::vector<dsg_handle*> hs;
    int B = 0, guided = 0, root_shift = 0, keep_last_tail = 0;
    const uint8_t* mask = nullptr;      // mask_local (one row), as set_window_cond takes it
    dsg_sample_args args;               // the queue's own; wargs: per lane, with the round's skip_timesteps (draw_base is the same for every
    std::vector<dsg_sample_args> wargs; // clip: the windows are told apart by the draw offsets)
    std::vector<SampleJob> sjobs;
    int (*cond)(dsg_handle* h, int B, const SlotWork* const* lane) = nullptr;      // the lane's slots -> style / audio / c_seed / c_seed_last
    // lane_init[i]: lane i starts its rounds through the edit table (k_clipq_x_in), else through k_x_in; lane_inp[i]: the table's constraint is
    // cut and the epilogue's inpainting is on.  lane_inp empty: decided per round, by whether a slot of the lane brings a mask
    std::vector<char> lane_inp, lane_init;
    // per lane: how the round's loop is started and run, and the storage of its noise table -- every slot its job's key and draw offsets
    struct Draws { std::vector<unsigned> keys, offs, starts; std::vector<int> holds; };
    std::vector<Draws> draws;
    std::vector<RunMode> modes;
    bool seed_last_written = false;     // variant 5: some round has put a job's snippet into c_seed_last
    int64_t steps_run = 0; std::vector<double> ms;      // since begin(): the step-loop length summed over the rounds, and per lane the time of its loops
    std::vector<const SlotWork*> lane;

    QueueRound(dsg_handle** hs_, int n, int B_, const uint8_t* mask_, int guided_, const dsg_sample_args& a, int root_shift_, int keep_last_tail_)
        : hs(hs_, hs_ + n), B(B_), guided(guided_ ? 1 : 0), root_shift(root_shift_ ? 1 : 0), keep_last_tail(keep_last_tail_ ? 1 : 0), mask(mask_),
          args(a), wargs(n, a), sjobs(n), lane_init(n, 0), draws(n), modes(n), ms(n, 0.0), lane(B_) {
        for (int i = 0; i < n; ++i) {
            dsg_handle::Queue& q = hs[i]->cq;
            q.slots_host.resize(B); q.edits_host.resize(B);
            q.scale_host.assign(B, 1.f);
            Draws& d = draws[i];
            d.keys.resize(4 * (size_t)B); d.offs.resize(B); d.starts.resize(B); d.holds.resize(B);
        }
    }
    // The lanes as the queue leaves them, on every path out of the one-shot call and at the session's close.  Variant 5: the rows of
    // c_seed_last now hold the jobs' snippets, so the lanes ask for dsg_set_seed_last again, as a fresh handle does
    void leave() {
        if (seed_last_written) for (dsg_handle* h : hs) h->seed_last_B = 0;
    }
    // in front of the rounds of one call: they follow whatever `stream` still does to the tensors they read
    int begin(void* stream) {
        steps_run = 0; ms.assign(hs.size(), 0.0);
        for (dsg_handle* h : hs) CHK(order_after(h, stream));
        return 0;
    }
    int run(const SlotWork* const* slots, void* stream) {      // slots: [B][lanes] (global slot s: lane s % n, position s / n)
        const int n = (int)hs.size(), n_sched = hs[0]->sched.n, variant5 = hs[0]->cfg.variant == 5;
        int s_r = n_sched;      // (the callers run no round without a live slot)
        for (int s = 0; s < n * B; ++s) if (slots[s]) s_r = std::min(s_r, slots[s]->skip);
        steps_run += n_sched - s_r;
        for (int i = 0; i < n; ++i) {
            dsg_handle* h = hs[i];
            dsg_handle::Queue& q = h->cq;
            Draws& d = draws[i];
            wargs[i].skip_timesteps = s_r;
            d.keys.assign(4 * (size_t)B, 0u);
            bool inp = !lane_inp.empty() && lane_inp[i];
            for (int b = 0; b < B; ++b) {
                const SlotWork* w = lane[b] = slots[(size_t)b * n + i];
                // a dead slot: a slot without edits and with hold 0 -- it starts as k_x_in starts it for the round's skip -- that hands nothing off
                EditSlot& e = q.edits_host[b];
                e = w ? w->ed : EditSlot{nullptr, nullptr, nullptr, 0, 0, 0.f, 0.f, 0, 0};
                // the start of the slot's chain -- do_q and the q_sample pair -- from the schedule of the lane that runs the slot: what k_x_in /
                // k_clip_x_in get on that lane for the slot's skip_timesteps
                const int skip = w ? w->skip : s_r, i0 = h->sched.n - skip - 1;
                e.qa = (float)h->sched.sqrt_ac[i0]; e.qb = (float)h->sched.sqrt_1mac[i0]; e.do_q = skip > 0 ? 1 : 0;
                q.slots_host[b] = HandoffSlot{nullptr, 0, 0, HQ_DEAD, 0};
                d.offs[b] = 0u; d.starts[b] = 0u; d.holds[b] = 0;
                if (!w) continue;
                const int c = w->c;
                e.c = c;
                q.scale_host[b] = w->job.scale;
                set_noise_key(&d.keys[4 * b], w->job.seed, w->job.stream_id);
                // what dsg_sample_clip alone consumes before window c; its step i is the round's loop index i + hold
                d.holds[b] = skip - s_r;
                d.starts[b] = (uint32_t)c * (uint32_t)(1 + w->n_run);
                d.offs[b] = d.starts[b] - (uint32_t)d.holds[b];
                q.slots_host[b] = HandoffSlot{w->clip, w->ed.n_out, c, (c == 0 ? HQ_FIRST : 0) | (c == w->job.K - 1 ? HQ_LAST : 0), 0};
                if (c == 0 && variant5) seed_last_written = true;
                if (lane_inp.empty() && w->ed.mask) inp = true;
            }
            if (variant5) h->seed_last_B = B;
            HIPCHK(hipMemcpyAsync(q.slots, q.slots_host.data(), (size_t)B * sizeof(HandoffSlot), hipMemcpyHostToDevice, h->stream));
            CHK(cond(h, B, lane.data()));
            CHK(set_window_cond(h, q.style, h->c_seed, q.audio, mask, 1, B, 0, guided ? q.scale_host.data() : nullptr, stream));
            if (inp || lane_init[i])
                HIPCHK(hipMemcpyAsync(q.edits, q.edits_host.data(), (size_t)B * sizeof(EditSlot), hipMemcpyHostToDevice, h->stream));
            if (inp) { CHK(queue_lane_ready(h, QL_INP)); CHK(launch_clip_inp_window_q(h, B)); }
            RunMode& m = modes[i];
            m.lanes = n; m.start = lane_init[i] ? RunMode::CLIPQ_X_IN : RunMode::X_IN; m.inpaint = inp ? B : 0;
            m.noise = NoiseTable{B, true, d.keys.data(), d.offs.data(), d.starts.data(), d.holds.data()};
        }
        for (int i = 0; i < n; ++i) CHK(sample_prepare(hs[i], &wargs[i], modes[i], B, stream, sjobs[i]));
        CHK(run_lanes(hs.data(), n, wargs.data(), sjobs.data()));
        for (int i = 0; i < n; ++i) {
            CHK(clip_window_timed(hs[i], sjobs[i], ms[i]));
            CHK(launch_handoff_q(hs[i], B, root_shift, keep_last_tail));
        }
        return 0;
    }
    // behind the rounds of one call (ran: there was one): what dsg_last_sample_ms and its kin report, and `stream` follows the lanes
    int end(bool ran, void* stream) {
        for (size_t i = 0; i < hs.size(); ++i) {
            if (ran) commit_report(hs[i], sjobs[i], (int)steps_run, ms[i]);
            CHK(order_before(hs[i], stream));
        }
        return 0;
    }
};

// dsg_sample_clip_queue_steps: the rounds of a plan (dsg_clip_queue_plan_steps: every clip a slot and a first round), every job's tensors
// read from the caller's memory.  What it adds to QueueRound:
//   slots      the plan's [round][slot] -> job table; a job stands on window c = round - its first round;
//   inputs     the round's style / audio (and, on a clip's first window, seed0 / seed_last) are copied slot by slot from where the caller keeps
//              them (cond_from_caller);
//   edits      NULL (dsg_sample_clip_queue), or one dsg_clip_edit per job -- the clip's constraint and / or the clip it is re-denoised from, in
//              the coordinates of the job's `out`.  Host tensors are staged on the lane that runs the job before the rounds start.  Lanes that
//              run a constrained job cut the constraint in every round (lane_inp), lanes that run a job with an init start every round through
//              the edit table (lane_init); a call without edits uploads no edit table and starts through k_x_in;
//   skips      skip_timesteps: NULL (dsg_sample_clip_queue_edit), or one entry per job (< 0: args->skip_timesteps).  When an entry differs
//              from the call's, the plan puts the deep jobs first and every lane starts every round through the edit table, which carries
//              do_q and the q_sample pair of the slot's own first timestep;
//   outputs    a host `out` is one copy per job at the end.
static int cond_from_caller(dsg_handle* h, int B, const SlotWork* const* lane) {
    const size_t sdi = h->cfg.style_dim_in, n_audio = (size_t)h->Ta * h->As, n_tail = (size_t)h->J * h->S;
    for (int b = 0; b < B; ++b) {
        const SlotWork* w = lane[b];
        if (!w) continue;
        CHK(upload(h, h->cq.style + b * sdi, w->job.style, sdi * sizeof(float)));
        CHK(upload(h, h->cq.audio + b * n_audio, w->job.audio + w->c * n_audio, n_audio * sizeof(float)));
        if (w->c != 0) continue;      // (later windows: the hand-off left y['seed'] in place)
        if (w->job.seed0) CHK(upload(h, h->c_seed + b * n_tail, w->job.seed0, n_tail * sizeof(float)));
        else HIPCHK(hipMemsetAsync(h->c_seed + b * n_tail, 0, n_tail * sizeof(float), h->stream));
        if (h->cfg.variant == 5) CHK(upload(h, h->c_seed_last + b * n_tail, w->job.seed_last, n_tail * sizeof(float)));
    }
    return 0;
}
extern "C" int dsg_sample_clip_queue_steps(dsg_handle** hs, int n, const dsg_clip_job* jobs, const dsg_clip_edit* edits, const int32_t* skip_timesteps,
                                           int n_jobs, int B, const uint8_t* mask_local, int guided, const dsg_sample_args* args, int root_shift,
                                           int keep_last_tail, void* stream) {
    if (!hs || !jobs || !args || n <= 0) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: bad argument");
    if (n > 16) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: at most 16 lanes (4 overlap on the hardware; put further clips into the lanes' batches)");
    if (n_jobs < 1) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: n_jobs < 1");
    CHK(clip_queue_check_lanes(hs, n, B, guided, args));
    const int variant5 = hs[0]->cfg.variant == 5;
    for (int j = 0; j < n_jobs; ++j) CHK(clip_queue_check_job(jobs[j], edits ? &edits[j] : nullptr, j, variant5));
    const int T = hs[0]->T, S = hs[0]->S, J = hs[0]->J;
    const int n_slots = n * B, keep = T - S;
    const int n_sched = hs[0]->sched.n;
    std::vector<int32_t> Ks(n_jobs), slot(n_jobs), first(n_jobs), n_runs(n_jobs);
    std::vector<SlotWork> work(n_jobs);
    bool own_skips = false;      // some job's skip differs from the call's: otherwise this IS dsg_sample_clip_queue_edit, launch for launch
    for (int j = 0; j < n_jobs; ++j) {
        SlotWork& w = work[j];
        w.job = jobs[j];
        Ks[j] = jobs[j].K;
        w.skip = skip_timesteps && skip_timesteps[j] >= 0 ? skip_timesteps[j] : args->skip_timesteps;
        if (w.skip < 0 || w.skip >= n_sched)
            return fail(DSG_E_INVALID, "dsg_sample_clip_queue: skip_timesteps out of range: job " + std::to_string(j) + " has skip_timesteps " + std::to_string(w.skip) +
                                       " outside [0, " + std::to_string(n_sched - 1) + "]");
        own_skips = own_skips || w.skip != args->skip_timesteps;
        n_runs[j] = w.n_run = n_sched - w.skip;
    }
    int32_t n_rounds = 0;
    CHK(dsg_clip_queue_plan_steps(Ks.data(), own_skips ? n_runs.data() : nullptr, n_jobs, n_slots, slot.data(), first.data(), &n_rounds, nullptr));
    std::vector<int> sched((size_t)n_rounds * n_slots, -1);      // [round][slot] -> job, -1: dead
    for (int j = 0; j < n_jobs; ++j)
        for (int c = 0; c < Ks[j]; ++c) sched[(size_t)(first[j] + c) * n_slots + slot[j]] = j;
    HIPCHK(hipSetDevice(hs[0]->cfg.device));
    // the clips: the caller's tensor where it is device memory, else a piece of ONE device buffer (lane 0's) and one copy per job at the end
    std::vector<size_t> n_clip(n_jobs);
    {
        size_t need = 0;
        for (int j = 0; j < n_jobs; ++j) {
            n_clip[j] = ((size_t)Ks[j] * keep - (keep_last_tail ? 0 : S)) * J;
            if (!is_device_ptr(jobs[j].out)) need += n_clip[j];
        }
        dsg_handle* h0 = hs[0];
        if (need > h0->clip_out_cap) { CHK(dalloc(h0, &h0->clip_out, need, false)); h0->clip_out_cap = need; }
        size_t at = 0;
        for (int j = 0; j < n_jobs; ++j) {
            if (is_device_ptr(jobs[j].out)) work[j].clip = jobs[j].out;
            else { work[j].clip = h0->clip_out + at; at += n_clip[j]; }
            work[j].ed = EditSlot{nullptr, nullptr, nullptr, (int)(n_clip[j] / J), 0, 0.f, 0.f, 0, 0};
        }
    }
    QueueRound rd(hs, n, B, mask_local, guided, *args, root_shift, keep_last_tail);
    struct QueueNow {      // the lanes leave the queue on every return path
        QueueRound& rd;
        ~QueueNow() { rd.leave(); }
    } queue_now{rd};
    rd.cond = cond_from_caller;
    rd.lane_inp.assign(n, 0);
    rd.lane_init.assign(n, own_skips ? 1 : 0);      // (per-clip skips: every lane starts every round through the table)
    for (int i = 0; i < n; ++i) CHK(queue_lane_ready(hs[i], own_skips ? QL_EDITS : 0));
    CHK(rd.begin(stream));
    // the edits: where each job's tensors are read on the device -- the caller's where they are device memory, else a piece of the staging of
    // the lane that runs the job (slot[j] % n), uploaded here on that lane's stream (the first round's sample_prepare drains it)
    if (edits) {
        const size_t r16 = 15;
        std::vector<size_t> need(n, 0);
        for (int j = 0; j < n_jobs; ++j) {
            const dsg_clip_edit& e = edits[j];
            const int i = slot[j] % n;
            if (e.inp_mask) rd.lane_inp[i] = 1;
            if (e.init_motion) rd.lane_init[i] = 1;
            if (e.inp_motion && !is_device_ptr(e.inp_motion)) need[i] += (n_clip[j] * sizeof(float) + r16) & ~r16;
            if (e.inp_mask && !is_device_ptr(e.inp_mask)) need[i] += (n_clip[j] + r16) & ~r16;
            if (e.init_motion && !is_device_ptr(e.init_motion)) need[i] += (n_clip[j] * sizeof(float) + r16) & ~r16;
        }
        for (int i = 0; i < n; ++i) {
            dsg_handle* h = hs[i];
            if (!rd.lane_inp[i] && !rd.lane_init[i]) continue;
            CHK(queue_lane_ready(h, QL_EDITS));
            if (need[i] > h->cq.stage_cap) {
                h->cq.stage_cap = 0;
                CHK(regrow(h, &h->cq.stage, need[i]));
                h->cq.stage_cap = need[i];
            }
        }
        std::vector<size_t> at(n, 0);
        for (int j = 0; j < n_jobs; ++j) {
            const dsg_clip_edit& e = edits[j];
            dsg_handle* h = hs[slot[j] % n];
            size_t& p = at[slot[j] % n];
            auto room = [&](size_t bytes, void** out) { *out = h->cq.stage + p; p += (bytes + r16) & ~r16; return 0; };
            EditSlot& ed = work[j].ed;
            CHK(staged(h, e.inp_motion, n_clip[j] * sizeof(float), room, (const void**)&ed.motion));
            CHK(staged(h, e.init_motion, n_clip[j] * sizeof(float), room, (const void**)&ed.init));
            CHK(staged(h, e.inp_mask, n_clip[j], room, (const void**)&ed.mask));
        }
    }
    std::vector<const SlotWork*> slots(n_slots);
    for (int r = 0; r < n_rounds; ++r) {      // (some slot is alive in every round of the plan)
        for (int s = 0; s < n_slots; ++s) {
            const int j = sched[(size_t)r * n_slots + s];
            slots[s] = j < 0 ? nullptr : &work[j];
            if (j >= 0) work[j].c = r - first[j];
        }
        CHK(rd.run(slots.data(), stream));
    }
    for (int j = 0; j < n_jobs; ++j)
        if (work[j].clip != jobs[j].out) CHK(from_dev(hs[slot[j] % n], jobs[j].out, work[j].clip, n_clip[j]));      // (on the stream of the lane that wrote it)
    return rd.end(true, stream);
}

extern "C" int dsg_sample_clip_queue_edit(dsg_handle** hs, int n, const dsg_clip_job* jobs, const dsg_clip_edit* edits, int n_jobs, int B,
                                          const uint8_t* mask_local, int guided, const dsg_sample_args* args, int root_shift, int keep_last_tail,
                                          void* stream) {
    return dsg_sample_clip_queue_steps(hs, n, jobs, edits, nullptr, n_jobs, B, mask_local, guided, args, root_shift, keep_last_tail, stream);
}
extern "C" int dsg_sample_clip_queue(dsg_handle** hs, int n, const dsg_clip_job* jobs, int n_jobs, int B, const uint8_t* mask_local, int guided,
                                     const dsg_sample_args* args, int root_shift, int keep_last_tail, void* stream) {
    return dsg_sample_clip_queue_edit(hs, n, jobs, nullptr, n_jobs, B, mask_local, guided, args, root_shift, keep_last_tail, stream);
}

// ---------------------------------------------------------------------------------------------------------
// Queue session (dsg_queue_*): the clip queue as an object that lives between rounds.  Jobs are submitted while it runs and a job's rows
// are in the caller's memory after the round that made them final.  What it adds to QueueRound:
//   slots      by priority, then first come, first served: at the start of a round the free slots, lowest first, take the waiting jobs,
//              highest priority and oldest ticket first, and a running job of a strictly lower priority is parked for one still waiting
//              (queue_place_round; dsg_queue_place_prio is the same code on the host, dsg_queue_place the rule with equal priorities); a job
//              stands on the window behind those it has done, in whichever slot it is;
//   inputs     a job's host tensors are copied into session-owned device memory at submit; the round's per-slot conditioning is gathered on
//              the device (cond_gathered: k_clipq_gather, one launch per lane);
//   edits      every lane starts every round through the edit table (k_clipq_x_in): a job with its own skip or an init motion may arrive in
//              any round.  The constraint is cut in the rounds in which a slot of the lane brings one;
//   outputs    a host `out` is fed from a session-owned device clip, the rows that became final copied after every round;
//   live jobs  (dsg_queue_submit_live / _append / _finish) get their windows one by one: a pending one is placed once it has a window, a
//              running one without a window to run is a dead slot for that round (its tail stays where its last window left it: the
//              hand-off picks the tail buffers per slot, by the window index), and K is unknown until finish.
// ---------------------------------------------------------------------------------------------------------
struct QBlock { void* p; size_t cap; };
struct QJob {
    SlotWork w;                       // every pointer as the device reads it: the caller's device tensors, or staging.  w.c: the windows done
    float* host_out = nullptr;        // the caller's host `out` (null: a device `out`, written by the hand-off itself)
    int state = DSG_JOB_PENDING, rows_ready = 0, rows_copied = 0, slot = -1, first_round = -1;
    std::vector<QBlock> blocks;       // the staging the job holds; back to the session's free list when it is done or cancelled
    // A live job (dsg_queue_submit_live): its windows arrive one by one (dsg_queue_append) until dsg_queue_finish says how many there are.
    // Until then w.job.K is INT32_MAX -- no window is the last one -- and w.ed.n_out is n_out(capacity); finish sets both to the clip's.
    // wins[c]: what window c runs on, every pointer as the device reads it; the round puts it into w.job.style / .scale and w.win_audio
    struct Win { const float* audio; const float* style; float scale; };
    bool live = false, finished = false;
    int capacity = 0;
    const float* style0 = nullptr;    // the job's own style and scale: what window 0 runs on unless it brings its own
    float scale0 = 1.f;
    std::vector<Win> wins;            // the windows given so far
    bool has_window() const { return !live || w.c < (int)wins.size(); }      // something to run in the next round
    // Priorities, park and resume.  Between two rounds the only device state a running job owns is the [S][J] tail its last window handed
    // off; everything else a round needs is rebuilt from the job.  A job that leaves its slot at a window boundary (state DSG_JOB_PARKED)
    // keeps that tail in `park`, a staging block of its own, and takes any slot of any lane later (SlotWork::resume, GQ_RESUME)
    int priority = 0, parks = 0;
    bool held = false;                // dsg_queue_park: not placed, and parked when a round finds it in a slot, until dsg_queue_resume
    float* park = nullptr;            // [S][J], written on the stream of lane park_lane; one of `blocks`
    int park_lane = 0;
    bool waiting() const { return (state == DSG_JOB_PENDING || state == DSG_JOB_PARKED) && !held && has_window(); }
};
struct dsg_queue {
    QueueRound rd;                    // the lanes, B, guided, args, root_shift, keep_last_tail; rd.mask: the session's device copy of mask_local
    std::vector<QJob> jobs;           // index = ticket
    std::vector<int64_t> slot_job;    // [n * B] -> ticket, -1: free
    size_t next_pending = 0;          // no ticket below it is pending or parked
    std::vector<hipEvent_t> ev_park;  // per lane: recorded behind the lane's latest park copy, for a job that resumes on another lane
    int64_t rounds_total = 0;
    std::multimap<size_t, void*> free_blocks;      // recycled staging, by capacity
    std::vector<void*> all_blocks;                 // every staging block ever allocated: released at close
};
// staging: blocks in power-of-two size classes (>= 256 bytes), recycled within the session, never freed between rounds (hipFree synchronises)
static int queue_take(dsg_queue* q, size_t bytes, QJob& jb, void** out) {
    size_t cap = 256;
    while (cap < bytes) cap <<= 1;
    void* p = nullptr;
    auto it = q->free_blocks.find(cap);
    if (it != q->free_blocks.end()) { p = it->second; q->free_blocks.erase(it); }
    else {
        if (hipMalloc(&p, cap) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DSG_E_RUNTIME, "dsg_queue_submit: out of device memory for " + std::to_string(cap) + " bytes of staging");
        }
        q->all_blocks.push_back(p);
    }
    jb.blocks.push_back(QBlock{p, cap});
    *out = p;
    return 0;
}
static void queue_give(dsg_queue* q, QJob& jb) {
    for (const QBlock& b : jb.blocks) q->free_blocks.emplace(b.cap, b.p);
    jb.blocks.clear();
}
static int queue_rows_ready(const dsg_queue* q, const QJob& jb) {
    const int S = q->rd.hs[0]->S, keep = q->rd.hs[0]->T - S, n_out = jb.w.ed.n_out;
    if (jb.w.c >= jb.w.job.K) return n_out;
    // window c leaves rows [c * keep - S, (c + 1) * keep - S) final (handoff_row), with keep_last_tail too: there only the LAST window writes
    // its closing S frames, and a job past its last window reports n_out above
    const int64_t r = (int64_t)jb.w.c * keep - S;
    return (int)std::max<int64_t>(0, std::min<int64_t>(n_out, r));
}

extern "C" int dsg_queue_place(const int32_t* K, const int32_t* arrive_round, int n_jobs, int n_slots, int32_t* slot, int32_t* first_round,
                               int32_t* n_rounds) {
    if (!K || !slot || !first_round || !n_rounds) return fail(DSG_E_INVALID, "dsg_queue_place: null argument");
    if (n_jobs < 1) return fail(DSG_E_INVALID, "dsg_queue_place: n_jobs < 1");
    if (n_slots < 1) return fail(DSG_E_INVALID, "dsg_queue_place: n_slots < 1");
    for (int j = 0; j < n_jobs; ++j) {
        if (K[j] < 1) return fail(DSG_E_INVALID, "dsg_queue_place: job " + std::to_string(j) + " has K < 1");
        if (arrive_round && (arrive_round[j] < 0 || (j > 0 && arrive_round[j] < arrive_round[j - 1])))
            return fail(DSG_E_INVALID, "dsg_queue_place: arrive_round must be non-negative and non-decreasing (job " + std::to_string(j) + ")");
    }
    // the session's rule, round by round: the free slots, lowest first, take the jobs that have arrived, oldest first.  (The session's
    // round counter advances only with a round that runs; an arrival later than the round at which every slot has gone idle is taken at
    // its own round here.)
    std::vector<int64_t> free_at(n_slots, 0);      // the round from which the slot is free
    int next = 0;
    int64_t r = 0, last = 0;
    while (next < n_jobs) {
        if (last <= r && arrive_round && arrive_round[next] > r) r = arrive_round[next];      // every slot idle: on to the next arrival
        for (int s = 0; s < n_slots && next < n_jobs; ++s) {
            if (free_at[s] > r) continue;
            if ((arrive_round ? arrive_round[next] : 0) > r) break;
            if (r + K[next] > 0x7fffffff) return fail(DSG_E_INVALID, "dsg_queue_place: more than 2^31 - 1 rounds");
            slot[next] = s; first_round[next] = (int32_t)r; free_at[s] = r + K[next]; last = std::max(last, free_at[s]); ++next;
        }
        ++r;
    }
    *n_rounds = (int32_t)last;
    return 0;
}

// The placement of one round, written once under dsg_queue_run and dsg_queue_place_prio.  wait: the jobs that may take a slot, in ticket
// order; slots: who holds each slot when the round starts.  (1) the waiting jobs are ordered by priority descending, ticket ascending;
// (2) the free slots, lowest first, take them in that order; (3) every waiting job still unplaced looks among the running jobs not placed
// in this round for the one of the lowest priority -- ties: first a job without a window to run, then the highest ticket -- and takes its
// slot if that priority is strictly lower, else the placement ends (the jobs behind it in the order have no higher priority).  moves: in
// the order made; parked >= 0: the job that leaves the slot.  With equal priorities (3) never moves anything and (1) + (2) is first come,
// first served.
struct PlaceWait { int64_t t; int32_t prio; };
struct PlaceSlot { int64_t t = -1; int32_t prio = 0; bool idle = false, fresh = false; };
struct PlaceMove { int64_t t; int slot; int64_t parked; };
static void queue_place_round(std::vector<PlaceWait>& wait, std::vector<PlaceSlot>& slots, std::vector<PlaceMove>& moves) {
    moves.clear();
    std::stable_sort(wait.begin(), wait.end(), [](const PlaceWait& a, const PlaceWait& b) { return a.prio > b.prio; });
    const int n_slots = (int)slots.size();
    size_t w = 0;
    for (int s = 0; s < n_slots && w < wait.size(); ++s) {
        if (slots[s].t >= 0) continue;
        moves.push_back(PlaceMove{wait[w].t, s, -1});
        slots[s] = PlaceSlot{wait[w].t, wait[w].prio, false, true};
        ++w;
    }
    for (; w < wait.size(); ++w) {
        int v = -1;
        for (int s = 0; s < n_slots; ++s) {
            const PlaceSlot& c = slots[s];
            if (c.t < 0 || c.fresh) continue;
            if (v < 0) { v = s; continue; }
            const PlaceSlot& b = slots[v];
            if (c.prio != b.prio ? c.prio < b.prio : c.idle != b.idle ? c.idle : c.t > b.t) v = s;
        }
        if (v < 0 || slots[v].prio >= wait[w].prio) break;
        moves.push_back(PlaceMove{wait[w].t, v, slots[v].t});
        slots[v] = PlaceSlot{wait[w].t, wait[w].prio, false, true};
    }
}

// The session's rounds on the host: nothing changes between two events -- an arrival, a job's last window -- so the rounds in between are
// stepped over.  done_round: the round of a job's last window; n_rounds: one past the last of them
extern "C" int dsg_queue_place_prio(const int32_t* K, const int32_t* arrive_round, const int32_t* priority, int n_jobs, int n_slots,
                                    int32_t* first_round, int32_t* done_round, int32_t* n_parks, int32_t* n_rounds) {
    if (!K || !first_round || !done_round || !n_parks || !n_rounds) return fail(DSG_E_INVALID, "dsg_queue_place_prio: null argument");
    if (n_jobs < 1) return fail(DSG_E_INVALID, "dsg_queue_place_prio: n_jobs < 1");
    if (n_slots < 1) return fail(DSG_E_INVALID, "dsg_queue_place_prio: n_slots < 1");
    for (int j = 0; j < n_jobs; ++j) {
        if (K[j] < 1) return fail(DSG_E_INVALID, "dsg_queue_place_prio: job " + std::to_string(j) + " has K < 1");
        if (arrive_round && (arrive_round[j] < 0 || (j > 0 && arrive_round[j] < arrive_round[j - 1])))
            return fail(DSG_E_INVALID, "dsg_queue_place_prio: arrive_round must be non-negative and non-decreasing (job " + std::to_string(j) + ")");
    }
    std::vector<int32_t> c(n_jobs, 0);      // windows done
    std::vector<int> at(n_jobs, -1);        // the slot a job runs in, -1: none
    std::vector<PlaceSlot> slots(n_slots);
    std::vector<PlaceWait> wait;
    std::vector<PlaceMove> moves;
    int arrived = 0, left = n_jobs;
    int64_t r = 0;
    for (int j = 0; j < n_jobs; ++j) { first_round[j] = -1; done_round[j] = -1; n_parks[j] = 0; }
    while (left > 0) {
        while (arrived < n_jobs && (arrive_round ? arrive_round[arrived] : 0) <= r) ++arrived;
        wait.clear();
        for (int j = 0; j < arrived; ++j)
            if (at[j] < 0 && c[j] < K[j]) wait.push_back(PlaceWait{j, priority ? priority[j] : 0});
        bool running = false;
        for (PlaceSlot& s : slots) { s.fresh = false; running = running || s.t >= 0; }
        if (!running && wait.empty()) { r = arrive_round[arrived]; continue; }      // every slot idle: on to the next arrival
        queue_place_round(wait, slots, moves);
        for (const PlaceMove& m : moves) {
            if (m.parked >= 0) { at[m.parked] = -1; ++n_parks[m.parked]; }
            at[m.t] = m.slot;
            if (c[m.t] == 0) first_round[m.t] = (int32_t)r;
        }
        int64_t dr = arrived < n_jobs ? (int64_t)arrive_round[arrived] - r : 0x7fffffff;
        for (const PlaceSlot& s : slots) if (s.t >= 0) dr = std::min<int64_t>(dr, K[s.t] - c[s.t]);
        r += dr;
        if (r > 0x7fffffff) return fail(DSG_E_INVALID, "dsg_queue_place_prio: more than 2^31 - 1 rounds");
        for (PlaceSlot& s : slots) {
            if (s.t < 0) continue;
            c[s.t] += (int32_t)dr;
            if (c[s.t] < K[s.t]) continue;
            done_round[s.t] = (int32_t)(r - 1); at[s.t] = -1; --left;
            s = PlaceSlot{};
        }
    }
    *n_rounds = (int32_t)r;
    return 0;
}

// A running job leaves its slot at a window boundary: the [S][J] tail its last window handed off -- clip_tail[(c - 1) & 1] of its position
// -- goes into a staging block of the job on the lane's stream, in front of the round's gather on that lane: whoever takes the slot
// overwrites c_seed and the tail only behind it in stream order.  The lane's park event is recorded behind the copy.  (c >= 1: a job is
// placed only with a window to run, so every job found in a slot when a round starts has handed a window off.)
static int queue_park_job(dsg_queue* q, int64_t t) {
    QJob& jb = q->jobs[t];
    QueueRound& rd = q->rd;
    const int n = (int)rd.hs.size(), lane = jb.slot % n, pos = jb.slot / n;
    dsg_handle* h = rd.hs[lane];
    const size_t n_tail = (size_t)h->S * h->J;
    if (!jb.park) {      // a recycled block may still be read by a round in flight (as dsg_queue_submit: the lanes are drained first)
        for (dsg_handle* hh : rd.hs) HIPCHK(hipStreamSynchronize(hh->stream));
        void* p = nullptr;
        CHK(queue_take(q, n_tail * sizeof(float), jb, &p));
        jb.park = (float*)p;
    }
    HIPCHK(hipMemcpyAsync(jb.park, h->clip_tail[(jb.w.c - 1) & 1] + pos * n_tail, n_tail * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipEventRecord(q->ev_park[lane], h->stream));
    q->slot_job[jb.slot] = -1;
    jb.park_lane = lane; jb.slot = -1; jb.state = DSG_JOB_PARKED; ++jb.parks;
    q->next_pending = std::min(q->next_pending, (size_t)t);
    return 0;
}

// the round's conditioning of a lane, gathered on the device from where the session keeps its jobs' tensors: the table, one launch
static int cond_gathered(dsg_handle* h, int B, const SlotWork* const* lane) {
    dsg_handle::Queue& q = h->cq;
    const size_t n_audio = (size_t)h->Ta * h->As;
    q.gather_host.resize(B);
    for (int b = 0; b < B; ++b) {
        const SlotWork* w = lane[b];
        q.gather_host[b] = w ? GatherSlot{w->job.style, w->win_audio ? w->win_audio : w->job.audio + w->c * n_audio, w->job.seed0, w->job.seed_last,
                                          GQ_LIVE | (w->c == 0 ? GQ_FIRST : 0) | (w->resume ? GQ_RESUME : 0), w->c, w->resume}
                             : GatherSlot{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr};
    }
    HIPCHK(hipMemcpyAsync(q.gather, q.gather_host.data(), (size_t)B * sizeof(GatherSlot), hipMemcpyHostToDevice, h->stream));
    GatherQArgs a;
    a.slots = q.gather; a.q_style = q.style; a.q_audio = q.audio; a.c_seed = h->c_seed; a.c_seed_last = h->c_seed_last;
    a.tail0 = h->clip_tail[0]; a.tail1 = h->clip_tail[1];
    a.B = B; a.sdi = h->cfg.style_dim_in; a.n_audio = h->Ta * h->As; a.n_seed = h->J * h->S; a.variant5 = h->cfg.variant == 5 ? 1 : 0; a.S = h->S;
    const size_t n = (size_t)B * ((a.sdi + 3) / 4 + (a.n_audio + 3) / 4 + (size_t)(a.variant5 ? 2 : 1) * ((a.n_seed + 3) / 4));
    hipLaunchKernelGGL(k_clipq_gather, dim3((int)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dsg_queue_open(dsg_handle** hs, int n, int B, const uint8_t* mask_local, int guided, const dsg_sample_args* args, int root_shift,
                              int keep_last_tail, dsg_queue** out) {
    if (!hs || !args || !out || n <= 0) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: bad argument");
    if (n > 16) return fail(DSG_E_INVALID, "dsg_sample_clip_queue: at most 16 lanes (4 overlap on the hardware; put further clips into the lanes' batches)");
    CHK(clip_queue_check_lanes(hs, n, B, guided, args));
    if (args->skip_timesteps < 0 || args->skip_timesteps >= hs[0]->sched.n)
        return fail(DSG_E_INVALID, "dsg_sample_clip_queue: skip_timesteps out of range: args has skip_timesteps " + std::to_string(args->skip_timesteps) +
                                   " outside [0, " + std::to_string(hs[0]->sched.n - 1) + "]");
    HIPCHK(hipSetDevice(hs[0]->cfg.device));
    for (int i = 0; i < n; ++i) CHK(queue_lane_ready(hs[i], QL_EDITS | QL_GATHER));
    unsigned char* mask_d = nullptr;      // the session's copy of mask_local (null: none was given)
    if (mask_local) {
        const size_t T = (size_t)hs[0]->T;
        if (hipMalloc((void**)&mask_d, T) != hipSuccess) { (void)hipGetLastError(); return fail(DSG_E_RUNTIME, "dsg_queue_open: out of device memory"); }
        const hipError_t e = hipMemcpy(mask_d, mask_local, T, is_device_ptr(mask_local) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(mask_d); HIPCHK(e); }
    }
    dsg_queue* q = new dsg_queue{QueueRound(hs, n, B, mask_d, guided, *args, root_shift, keep_last_tail)};
    q->rd.cond = cond_gathered;
    q->rd.lane_init.assign(n, 1);      // (lane_inp stays empty: per round)
    q->slot_job.assign((size_t)n * B, -1);
    for (int i = 0; i < n; ++i) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            for (hipEvent_t e : q->ev_park) (void)hipEventDestroy(e);
            if (mask_d) (void)hipFree(mask_d);
            delete q;
            return fail(DSG_E_RUNTIME, "dsg_queue_open: hipEventCreate failed");
        }
        q->ev_park.push_back(ev);
    }
    for (int i = 0; i < n; ++i) hs[i]->owner = q;
    *out = q;
    return 0;
}

// dsg_queue_submit and dsg_queue_submit_live (n_given >= 0: job->K is the capacity and job->audio holds the first n_given windows)
static int queue_submit(dsg_queue* q, const dsg_clip_job* job, const dsg_clip_edit* edit, int skip_timesteps, int n_given, int64_t* ticket, void* stream) {
    if (!q || !job || !ticket) return fail(DSG_E_INVALID, "dsg_queue_submit: null argument");
    dsg_handle* h0 = q->rd.hs[0];
    const int64_t t = (int64_t)q->jobs.size();
    const bool live = n_given >= 0;
    CHK(clip_queue_check_job(*job, edit, t, h0->cfg.variant == 5, live && n_given == 0));
    if (live && n_given > job->K)
        return fail(DSG_E_INVALID, "dsg_queue_submit_live: job " + std::to_string(t) + " brings " + std::to_string(n_given) + " windows for a capacity of " + std::to_string(job->K));
    const int n_sched = h0->sched.n, skip = skip_timesteps >= 0 ? skip_timesteps : q->rd.args.skip_timesteps;
    if (skip < 0 || skip >= n_sched)
        return fail(DSG_E_INVALID, "dsg_sample_clip_queue: skip_timesteps out of range: job " + std::to_string(t) + " has skip_timesteps " + std::to_string(skip) +
                                   " outside [0, " + std::to_string(n_sched - 1) + "]");
    const int T = h0->T, S = h0->S, J = h0->J, keep = T - S;
    const size_t n_tail = (size_t)J * S, n_audio = (size_t)h0->Ta * h0->As;
    if ((int64_t)job->K * keep > 0x7fffffff) return fail(DSG_E_INVALID, "dsg_queue_submit: job " + std::to_string(t) + " has more than 2^31 - 1 rows");
    HIPCHK(hipSetDevice(h0->cfg.device));
    QJob jb;
    SlotWork& w = jb.w;
    w.job = *job;
    const int n_out = job->K * keep - (q->rd.keep_last_tail ? 0 : S);
    w.skip = skip; w.n_run = n_sched - skip;
    const size_t n_clip = (size_t)n_out * J;
    w.ed = EditSlot{nullptr, nullptr, nullptr, n_out, 0, 0.f, 0.f, 0, 0};
    // a recycled block may still be read by a round in flight on some lane (HIP launches return early): the lanes are drained before the
    // first host tensor is written over one.  They are idle whenever the step loop went through the AQL queues, so this waits for nothing
    bool drained = false;
    auto room = [&](size_t bytes, void** p) -> int {
        if (!drained) { for (dsg_handle* h : q->rd.hs) HIPCHK(hipStreamSynchronize(h->stream)); drained = true; }
        return queue_take(q, bytes, jb, p);
    };
    int rc = 0;
    if (!rc) rc = staged(h0, job->style, (size_t)h0->cfg.style_dim_in * sizeof(float), room, (const void**)&w.job.style);
    if (!rc) rc = staged(h0, job->seed0, n_tail * sizeof(float), room, (const void**)&w.job.seed0);
    if (!rc) rc = staged(h0, job->seed_last, n_tail * sizeof(float), room, (const void**)&w.job.seed_last);
    const int n_windows = live ? n_given : job->K;      // the windows job->audio holds
    if (n_windows == 0) w.job.audio = nullptr;
    else if (!rc) rc = staged(h0, job->audio, (size_t)n_windows * n_audio * sizeof(float), room, (const void**)&w.job.audio);
    if (!rc && edit) {
        rc = staged(h0, edit->inp_motion, n_clip * sizeof(float), room, (const void**)&w.ed.motion);
        if (!rc) rc = staged(h0, edit->init_motion, n_clip * sizeof(float), room, (const void**)&w.ed.init);
        if (!rc) rc = staged(h0, edit->inp_mask, n_clip, room, (const void**)&w.ed.mask);
    }
    if (!rc) {
        if (is_device_ptr(job->out)) w.clip = job->out;
        else {
            void* p = nullptr;
            rc = queue_take(q, n_clip * sizeof(float), jb, &p);
            w.clip = (float*)p; jb.host_out = job->out;
        }
    }
    // the caller's host buffers are free on return: the copies above have landed
    if (!rc && drained && hipStreamSynchronize(h0->stream) != hipSuccess) { (void)hipGetLastError(); rc = fail(DSG_E_RUNTIME, "dsg_queue_submit: staging copy failed"); }
    if (rc) { queue_give(q, jb); return rc; }      // the session is as it was (the blocks taken so far wait in its free list)
    // device tensors of the job are read where they are: whatever `stream` still does to them comes first on every lane
    for (dsg_handle* h : q->rd.hs) CHK(order_after(h, stream));
    if (live) {
        jb.live = true; jb.capacity = job->K; jb.style0 = w.job.style; jb.scale0 = job->scale;
        for (int c = 0; c < n_given; ++c) jb.wins.push_back(QJob::Win{w.job.audio + c * n_audio, jb.style0, jb.scale0});
        w.job.K = 0x7fffffff;
    }
    q->jobs.push_back(std::move(jb));
    *ticket = t;
    return 0;
}
extern "C" int dsg_queue_submit(dsg_queue* q, const dsg_clip_job* job, const dsg_clip_edit* edit, int skip_timesteps, int64_t* ticket, void* stream) {
    return queue_submit(q, job, edit, skip_timesteps, -1, ticket, stream);
}
extern "C" int dsg_queue_submit_live(dsg_queue* q, const dsg_clip_job* job, int n_given, int skip_timesteps, int64_t* ticket, void* stream) {
    if (n_given < 0) return fail(DSG_E_INVALID, "dsg_queue_submit_live: n_given < 0");
    return queue_submit(q, job, nullptr, skip_timesteps, n_given, ticket, stream);
}

// The end of a live job whose given windows have all run (dsg_queue_finish after the fact): nothing is left to run.  Without keep_last_tail
// every row of the clip is written and delivered already.  With it the closing S rows are the slot's tail -- [S][J], the values handoff_row
// stored for f >= keep after the shift, which are the values the last window would have written to the clip had it known it was the last;
// window K - 1 wrote clip_tail[(K - 1) & 1] -- copied on the lane's stream into the clip and on to a host `out`.  The lane is drained: the
// call has no stream of the caller's to order a device `out` before.  A PARKED job holds no slot: its tail is the parked block -- the same
// values, copied when it left its slot -- read on the stream of the lane that wrote it
static int queue_finish_late(dsg_queue* q, QJob& jb) {
    const QueueRound& rd = q->rd;
    const int n = (int)rd.hs.size(), J = rd.hs[0]->J, S = rd.hs[0]->S, keep = rd.hs[0]->T - S, K = jb.w.job.K;
    const bool parked = jb.state == DSG_JOB_PARKED;
    dsg_handle* h = rd.hs[parked ? jb.park_lane : jb.slot % n];
    HIPCHK(hipSetDevice(h->cfg.device));
    if (rd.keep_last_tail) {
        const float* tail = parked ? jb.park : h->clip_tail[(K - 1) & 1] + (size_t)(jb.slot / n) * S * J;
        HIPCHK(hipMemcpyAsync(jb.w.clip + ((size_t)K * keep - S) * J, tail, (size_t)S * J * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    jb.rows_ready = jb.w.ed.n_out;
    if (jb.host_out && jb.rows_ready > jb.rows_copied) {
        const size_t at = (size_t)jb.rows_copied * J, cnt = (size_t)(jb.rows_ready - jb.rows_copied) * J;
        HIPCHK(hipMemcpyAsync(jb.host_out + at, jb.w.clip + at, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        jb.rows_copied = jb.rows_ready;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    jb.state = DSG_JOB_DONE;
    queue_give(q, jb);
    jb.park = nullptr;
    if (!parked) q->slot_job[jb.slot] = -1;
    return 0;
}
extern "C" int dsg_queue_finish(dsg_queue* q, int64_t ticket) {
    if (!q) return fail(DSG_E_INVALID, "dsg_queue_finish: null queue");
    if (ticket < 0 || ticket >= (int64_t)q->jobs.size()) return fail(DSG_E_INVALID, "dsg_queue_finish: no such ticket: " + std::to_string(ticket));
    QJob& jb = q->jobs[ticket];
    if (!jb.live) return fail(DSG_E_INVALID, "dsg_queue_finish: ticket " + std::to_string(ticket) + " is not a live job");
    if (jb.finished || jb.state == DSG_JOB_DONE || jb.state == DSG_JOB_CANCELLED) return 0;      // nothing left to finish
    jb.finished = true;
    const int K = (int)jb.wins.size(), S = q->rd.hs[0]->S, keep = q->rd.hs[0]->T - S;
    if (K == 0) {      // no window was ever given (so it never took a slot): there is no clip
        jb.state = DSG_JOB_CANCELLED;
        queue_give(q, jb);
        return 0;
    }
    jb.w.job.K = K;
    jb.w.ed.n_out = K * keep - (q->rd.keep_last_tail ? 0 : S);
    if ((jb.state == DSG_JOB_RUNNING || jb.state == DSG_JOB_PARKED) && jb.w.c >= K) return queue_finish_late(q, jb);
    return 0;      // windows still to run: the last of them runs with HQ_LAST and the job is done after that round
}
extern "C" int dsg_queue_append(dsg_queue* q, int64_t ticket, const dsg_queue_window* wins, int n, void* stream) {
    if (!q || !wins) return fail(DSG_E_INVALID, "dsg_queue_append: null argument");
    const std::string tk = std::to_string(ticket);
    if (ticket < 0 || ticket >= (int64_t)q->jobs.size()) return fail(DSG_E_INVALID, "dsg_queue_append: no such ticket: " + tk);
    QJob& jb = q->jobs[ticket];
    if (!jb.live) return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + " is not a live job");
    if (jb.state == DSG_JOB_DONE) return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + " is done");
    if (jb.state == DSG_JOB_CANCELLED) return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + " is cancelled");
    if (jb.finished) return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + " is finished");
    if (n < 1) return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + ": n < 1");
    if ((int64_t)jb.wins.size() + n > jb.capacity)
        return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + ": " + std::to_string(jb.wins.size()) + " + " + std::to_string(n) +
                                   " windows exceed the capacity of " + std::to_string(jb.capacity));
    for (int i = 0; i < n; ++i) {
        if (!wins[i].audio) return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + ": window " + std::to_string(i) + " has a null audio");
        if ((wins[i].flags & DSG_WIN_LAST) && i != n - 1)
            return fail(DSG_E_INVALID, "dsg_queue_append: ticket " + tk + ": DSG_WIN_LAST on window " + std::to_string(i) + " of " + std::to_string(n) + ": only the last entry may carry it");
    }
    dsg_handle* h0 = q->rd.hs[0];
    HIPCHK(hipSetDevice(h0->cfg.device));
    const size_t n_audio = (size_t)h0->Ta * h0->As, n_blocks = jb.blocks.size();
    bool drained = false;      // (as dsg_queue_submit: a recycled block may still be read by a round in flight)
    auto room = [&](size_t bytes, void** p) -> int {
        if (!drained) { for (dsg_handle* h : q->rd.hs) HIPCHK(hipStreamSynchronize(h->stream)); drained = true; }
        return queue_take(q, bytes, jb, p);
    };
    std::vector<QJob::Win> add(n);
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) {
        const QJob::Win* prev = i > 0 ? &add[i - 1] : jb.wins.empty() ? nullptr : &jb.wins.back();
        QJob::Win& wn = add[i];
        rc = staged(h0, wins[i].audio, n_audio * sizeof(float), room, (const void**)&wn.audio);
        if (!rc && wins[i].style) rc = staged(h0, wins[i].style, (size_t)h0->cfg.style_dim_in * sizeof(float), room, (const void**)&wn.style);
        else wn.style = prev ? prev->style : jb.style0;
        wn.scale = (wins[i].flags & DSG_WIN_SCALE) && q->rd.guided ? wins[i].scale : prev ? prev->scale : jb.scale0;
    }
    if (!rc && drained && hipStreamSynchronize(h0->stream) != hipSuccess) { (void)hipGetLastError(); rc = fail(DSG_E_RUNTIME, "dsg_queue_append: staging copy failed"); }
    if (rc) {      // the job is as it was: the blocks taken here go back to the free list
        for (size_t b = n_blocks; b < jb.blocks.size(); ++b) q->free_blocks.emplace(jb.blocks[b].cap, jb.blocks[b].p);
        jb.blocks.resize(n_blocks);
        return rc;
    }
    for (dsg_handle* h : q->rd.hs) CHK(order_after(h, stream));
    jb.wins.insert(jb.wins.end(), add.begin(), add.end());
    return (wins[n - 1].flags & DSG_WIN_LAST) ? dsg_queue_finish(q, ticket) : 0;
}

extern "C" int dsg_queue_run(dsg_queue* q, int max_rounds, int* rounds_run, void* stream) {
    if (rounds_run) *rounds_run = 0;
    if (!q) return fail(DSG_E_INVALID, "dsg_queue_run: null queue");
    QueueRound& rd = q->rd;
    dsg_handle** hs = rd.hs.data();
    const int n = (int)rd.hs.size(), n_slots = n * rd.B, J = hs[0]->J;
    HIPCHK(hipSetDevice(hs[0]->cfg.device));
    CHK(rd.begin(stream));
    std::vector<const SlotWork*> slots(n_slots);
    std::vector<PlaceWait> wait;
    std::vector<PlaceSlot> held_by(n_slots);
    std::vector<PlaceMove> moves;
    int done = 0;
    while (max_rounds <= 0 || done < max_rounds) {
        // a running job the caller holds (dsg_queue_park) leaves its slot
        for (int s = 0; s < n_slots; ++s)
            if (q->slot_job[s] >= 0 && q->jobs[q->slot_job[s]].held) CHK(queue_park_job(q, q->slot_job[s]));
        // placement (queue_place_round): the waiting jobs -- pending or parked, not held, with a window to run -- by priority, then ticket;
        // free slots first, then the slots of running jobs of a strictly lower priority, which are parked.  (A live job without a window
        // cannot be placed: the tickets behind it pass it.)  With equal priorities: the free slots, lowest first, take the oldest tickets
        while (q->next_pending < q->jobs.size() && q->jobs[q->next_pending].state != DSG_JOB_PENDING && q->jobs[q->next_pending].state != DSG_JOB_PARKED)
            ++q->next_pending;
        wait.clear();
        for (size_t t = q->next_pending; t < q->jobs.size(); ++t)
            if (q->jobs[t].waiting()) wait.push_back(PlaceWait{(int64_t)t, q->jobs[t].priority});
        for (int s = 0; s < n_slots; ++s) {
            const int64_t t = q->slot_job[s];
            held_by[s] = t < 0 ? PlaceSlot{} : PlaceSlot{t, q->jobs[t].priority, !q->jobs[t].has_window(), false};
        }
        queue_place_round(wait, held_by, moves);
        for (const PlaceMove& m : moves) {
            if (m.parked >= 0) CHK(queue_park_job(q, m.parked));
            QJob& jb = q->jobs[m.t];
            if (jb.state == DSG_JOB_PARKED) {      // its tail goes into the new slot with the round's gather, behind the copy that parked it
                jb.w.resume = jb.park;
                if (m.slot % n != jb.park_lane) HIPCHK(hipStreamWaitEvent(hs[m.slot % n]->stream, q->ev_park[jb.park_lane], 0));
            } else jb.first_round = (int)q->rounds_total;
            jb.state = DSG_JOB_RUNNING; jb.slot = m.slot;
            q->slot_job[m.slot] = m.t;
        }
        // a running live job without a window to run sits the round out: a dead slot, whose c_seed rows, tail and state stay
        bool alive = false;
        for (int s = 0; s < n_slots; ++s) {
            slots[s] = nullptr;
            if (q->slot_job[s] < 0) continue;
            QJob& jb = q->jobs[q->slot_job[s]];
            if (!jb.has_window()) continue;
            if (jb.live) {      // the window it stands on brings its own audio, style and scale
                const QJob::Win& wn = jb.wins[jb.w.c];
                jb.w.win_audio = wn.audio; jb.w.job.style = wn.style; jb.w.job.scale = wn.scale;
            }
            slots[s] = &jb.w;
            alive = true;
        }
        if (!alive) break;      // no slot has a window to run, no pending job can be placed
        CHK(rd.run(slots.data(), stream));
        // the round's windows are handed off: the rows that became final go to the callers' host memory, on the stream of the lane that
        // wrote them; finished jobs leave their slots
        std::vector<char> copied(n, 0);
        for (int s = 0; s < n_slots; ++s) {
            const int64_t t = q->slot_job[s];
            if (!slots[s]) continue;
            QJob& jb = q->jobs[t];
            ++jb.w.c;
            jb.w.resume = nullptr;      // (its tail is the slot's again)
            jb.rows_ready = queue_rows_ready(q, jb);
            if (jb.host_out && jb.rows_ready > jb.rows_copied) {
                const size_t at = (size_t)jb.rows_copied * J, cnt = (size_t)(jb.rows_ready - jb.rows_copied) * J;
                HIPCHK(hipMemcpyAsync(jb.host_out + at, jb.w.clip + at, cnt * sizeof(float), hipMemcpyDeviceToHost, hs[s % n]->stream));
                jb.rows_copied = jb.rows_ready;
                copied[s % n] = 1;
            }
        }
        for (int i = 0; i < n; ++i) if (copied[i]) HIPCHK(hipStreamSynchronize(hs[i]->stream));
        for (int s = 0; s < n_slots; ++s) {
            const int64_t t = q->slot_job[s];
            if (t < 0 || q->jobs[t].w.c < q->jobs[t].w.job.K) continue;
            q->jobs[t].state = DSG_JOB_DONE;
            queue_give(q, q->jobs[t]);
            q->slot_job[s] = -1;
        }
        ++q->rounds_total; ++done;
    }
    CHK(rd.end(done > 0, stream));
    if (rounds_run) *rounds_run = done;
    return 0;
}

extern "C" int dsg_queue_job(dsg_queue* q, int64_t ticket, dsg_queue_job_info* info) {
    if (!q || !info) return fail(DSG_E_INVALID, "dsg_queue_job: null argument");
    if (ticket < 0 || ticket >= (int64_t)q->jobs.size()) return fail(DSG_E_INVALID, "dsg_queue_job: no such ticket: " + std::to_string(ticket));
    const QJob& jb = q->jobs[ticket];
    memset(info, 0, sizeof *info);
    info->state = jb.state; info->windows_done = jb.w.c; info->rows_ready = jb.rows_ready; info->slot = jb.slot; info->first_round = jb.first_round;
    if (jb.live) { info->windows_given = (int32_t)jb.wins.size(); info->live = DSG_JOB_LIVE | (jb.finished ? DSG_JOB_FINISHED : 0); }
    if (jb.held && jb.state != DSG_JOB_DONE && jb.state != DSG_JOB_CANCELLED) info->live |= DSG_JOB_HELD;
    info->reserved[0] = jb.parks;
    return 0;
}
extern "C" int dsg_queue_info(dsg_queue* q, int64_t* rounds_total, int* n_pending, int* n_running) {
    if (!q) return fail(DSG_E_INVALID, "dsg_queue_info: null queue");
    int pend = 0, run = 0;
    for (size_t t = q->next_pending; t < q->jobs.size(); ++t) pend += q->jobs[t].state == DSG_JOB_PENDING || q->jobs[t].state == DSG_JOB_PARKED;
    for (int64_t t : q->slot_job) run += t >= 0;
    if (rounds_total) *rounds_total = q->rounds_total;
    if (n_pending) *n_pending = pend;
    if (n_running) *n_running = run;
    return 0;
}
extern "C" int dsg_queue_cancel(dsg_queue* q, int64_t ticket) {
    if (!q) return fail(DSG_E_INVALID, "dsg_queue_cancel: null queue");
    if (ticket < 0 || ticket >= (int64_t)q->jobs.size()) return fail(DSG_E_INVALID, "dsg_queue_cancel: no such ticket: " + std::to_string(ticket));
    QJob& jb = q->jobs[ticket];
    if (jb.state == DSG_JOB_DONE || jb.state == DSG_JOB_CANCELLED) return 0;      // nothing left to cancel
    if (jb.state == DSG_JOB_RUNNING) q->slot_job[jb.slot] = -1;                    // dead from the next round on; the rows written so far stay
    jb.state = DSG_JOB_CANCELLED;      // (a parked job holds no slot)
    queue_give(q, jb);      // (dsg_queue_submit drains the lanes before it writes over a recycled block, a parked tail included)
    jb.park = nullptr;
    return 0;
}
// dsg_queue_set_priority / _park / _resume: the job's word for the next placement; nothing happens on the device before dsg_queue_run
static int queue_ticket(dsg_queue* q, int64_t ticket, const char* who, QJob** jb) {
    if (!q) return fail(DSG_E_INVALID, std::string(who) + ": null queue");
    if (ticket < 0 || ticket >= (int64_t)q->jobs.size()) return fail(DSG_E_INVALID, std::string(who) + ": no such ticket: " + std::to_string(ticket));
    *jb = &q->jobs[ticket];
    return 0;
}
extern "C" int dsg_queue_set_priority(dsg_queue* q, int64_t ticket, int32_t priority) {
    QJob* jb = nullptr;
    CHK(queue_ticket(q, ticket, "dsg_queue_set_priority", &jb));
    if (jb->state != DSG_JOB_DONE && jb->state != DSG_JOB_CANCELLED) jb->priority = priority;
    return 0;
}
extern "C" int dsg_queue_park(dsg_queue* q, int64_t ticket) {
    QJob* jb = nullptr;
    CHK(queue_ticket(q, ticket, "dsg_queue_park", &jb));
    if (jb->state != DSG_JOB_DONE && jb->state != DSG_JOB_CANCELLED) jb->held = true;      // (a parked or held job: nothing changes)
    return 0;
}
extern "C" int dsg_queue_resume(dsg_queue* q, int64_t ticket) {
    QJob* jb = nullptr;
    CHK(queue_ticket(q, ticket, "dsg_queue_resume", &jb));
    jb->held = false;
    return 0;
}
extern "C" int dsg_queue_close(dsg_queue* q) {
    if (!q) return 0;
    (void)hipSetDevice(q->rd.hs[0]->cfg.device);
    for (dsg_handle* h : q->rd.hs) {
        (void)hipStreamSynchronize(h->stream);
        h->owner = nullptr;
    }
    q->rd.leave();
    for (hipEvent_t e : q->ev_park) (void)hipEventDestroy(e);
    for (void* p : q->all_blocks) (void)hipFree(p);
    if (q->rd.mask) (void)hipFree((void*)q->rd.mask);
    delete q;
    return 0;
}

extern "C" int dsg_sync(dsg_handle* h) {
    if (!h) return fail(DSG_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int dsg_last_sample_ms(dsg_handle* h, float* ms, int* n_steps) {
    if (!h || !ms) return fail(DSG_E_INVALID, "null argument");
    if (!h->last.sampled) return fail(DSG_E_STATE, "no dsg_sample has run");
    HIPCHK(hipEventSynchronize(h->ev_t1));
    if (h->last.host_ms >= 0.0) *ms = (float)h->last.host_ms;      // the AQL clock, or the sum over a clip's windows / a queue's rounds
    else HIPCHK(hipEventElapsedTime(ms, h->ev_t0, h->ev_t1));
    if (n_steps) *n_steps = h->last.steps;
    return 0;
}
// how the step loop of the last dsg_sample was submitted: 0 = HIP launches, 1 = hand-written AQL packets, 2 = hipGraph replay
extern "C" int dsg_last_sample_path(dsg_handle* h, int* path) {
    if (!h || !path) return fail(DSG_E_INVALID, "null argument");
    if (!h->last.sampled) return fail(DSG_E_STATE, "no dsg_sample has run");
    *path = h->last.path;
    return 0;
}
// 1 when the packets of the last dsg_sample's loop carried no acquire / release fences (AQL paths only)
extern "C" int dsg_last_sample_fence_free(dsg_handle* h, int* fence_free) {
    if (!h || !fence_free) return fail(DSG_E_INVALID, "null argument");
    if (!h->last.sampled) return fail(DSG_E_STATE, "no dsg_sample has run");
    *fence_free = h->last.nofence ? 1 : 0;
    return 0;
}

// the framework's noise stream as a tensor (what the fused sampler consumes for draw index `draw`): out [B, J, 1, T], device
// memory (written on `stream`) or host memory (generated on the device, copied back, synchronous)
static int noise_tensor(float* out, int B, int J, int T, NoiseKey nk, const unsigned* keys, uint32_t draw, void* stream) {
    const int Jq = rup(J, 4);
    const size_t n = (size_t)B * T * (Jq / 4), bytes = (size_t)B * J * T * sizeof(float);
    const bool dev = is_device_ptr(out);
    float* dst = out;
    if (!dev) HIPCHK(hipMalloc((void**)&dst, bytes));
    hipLaunchKernelGGL(k_noise, dim3((int)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, dst, B, J, Jq, T, nk, keys, draw);
    hipError_t e = hipGetLastError();
    if (!dev) {          // host output: the temporary is released on every path
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e == hipSuccess) e = hipMemcpy(out, dst, bytes, hipMemcpyDeviceToHost);
        (void)hipFree(dst);
    }
    if (e != hipSuccess) return fail(DSG_E_RUNTIME, std::string("dsg_noise: ") + hipGetErrorString(e));
    return 0;
}
extern "C" int dsg_noise(float* out, int B, int J, int T, uint64_t seed, uint64_t stream_id, uint32_t draw, void* stream) {
    if (!out || B <= 0 || J <= 0 || T <= 0) return fail(DSG_E_INVALID, "dsg_noise: bad argument");
    NoiseKey nk;
    nk.k0 = (unsigned)(seed & 0xffffffffu); nk.k1 = (unsigned)(seed >> 32);
    nk.s0 = (unsigned)(stream_id & 0xffffffffu); nk.s1 = (unsigned)(stream_id >> 32);
    return noise_tensor(out, B, J, T, nk, nullptr, draw, stream);
}
// dsg_noise with per-element streams: element b of out [B, J, 1, T] is draw `draw` of (seeds[b], stream_ids[b]) with the batch term of the
// counter 0 -- bit for bit dsg_noise(B = 1, seeds[b], stream_ids[b], draw), and what the fused loops consume for that draw index on a handle
// with dsg_set_noise_streams.  seeds / stream_ids: HOST uint64[B]; a NULL one reads as zeros
extern "C" int dsg_noise_streams(float* out, int B, int J, int T, const uint64_t* seeds, const uint64_t* stream_ids, uint32_t draw, void* stream) {
    if (!out || B <= 0 || J <= 0 || T <= 0) return fail(DSG_E_INVALID, "dsg_noise_streams: bad argument");
    std::vector<unsigned> hk(4 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        const uint64_t sd = seeds ? seeds[b] : 0, id = stream_ids ? stream_ids[b] : 0;
        hk[4 * b] = (unsigned)(sd & 0xffffffffu); hk[4 * b + 1] = (unsigned)(sd >> 32);
        hk[4 * b + 2] = (unsigned)(id & 0xffffffffu); hk[4 * b + 3] = (unsigned)(id >> 32);
    }
    unsigned* keys = nullptr;
    HIPCHK(hipMalloc((void**)&keys, hk.size() * sizeof(unsigned)));
    hipError_t e = hipMemcpy(keys, hk.data(), hk.size() * sizeof(unsigned), hipMemcpyHostToDevice);      // (synchronous: `hk` is free after it)
    int rc = 0;
    if (e != hipSuccess) rc = fail(DSG_E_RUNTIME, std::string("dsg_noise_streams: ") + hipGetErrorString(e));
    else {
        const NoiseKey nk = {0, 0, 0, 0};
        rc = noise_tensor(out, B, J, T, nk, keys, draw, stream);
        // the table is released once the kernel that reads it has run (a device `out` is written on `stream`, as by dsg_noise)
        if (rc == 0 && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = fail(DSG_E_RUNTIME, "dsg_noise_streams: synchronize");
    }
    (void)hipFree(keys);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------
// stand-alone fused sampler arithmetic on caller tensors
// ---------------------------------------------------------------------------------------------------------
static int elementwise(float* out, const float* p, const float* q, const float* z, const float* a, const float* c,
                       const float* s, int B, int64_t per, void* stream) {
    if (!out || !p || !a || B <= 0 || per <= 0) return fail(DSG_E_INVALID, "elementwise: bad argument");
    if (!is_device_ptr(out) || !is_device_ptr(p) || (q && !is_device_ptr(q)) || (z && !is_device_ptr(z)))
        return fail(DSG_E_INVALID, "elementwise kernels take device tensors");
    float* coef = nullptr;
    HIPCHK(hipMalloc((void**)&coef, 3 * B * sizeof(float)));
    std::vector<float> hc(3 * B, 0.f);
    for (int b = 0; b < B; ++b) { hc[b] = a[b]; hc[B + b] = c ? c[b] : 0.f; hc[2 * B + b] = s ? s[b] : 0.f; }
    HIPCHK(hipMemcpy(coef, hc.data(), hc.size() * sizeof(float), hipMemcpyHostToDevice));
    const size_t n = (size_t)B * per;
    hipLaunchKernelGGL(k_axpbypcz, dim3((int)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                       out, p, q, z, coef, coef + B, coef + 2 * B, B, (size_t)per);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipFree(coef));
    return 0;
}
extern "C" int dsg_q_sample(float* out, const float* x_start, const float* noise, const float* sqrt_ac,
                            const float* sqrt_1mac, int B, int64_t per, void* stream) {
    return elementwise(out, x_start, noise, nullptr, sqrt_ac, sqrt_1mac, nullptr, B, per, stream);
}
extern "C" int dsg_predict_xstart_from_eps(float* out, const float* x_t, const float* eps, const float* sqrt_recip,
                                           const float* sqrt_recipm1, int B, int64_t per, void* stream) {
    std::vector<float> neg(B);
    for (int b = 0; b < B; ++b) neg[b] = -sqrt_recipm1[b];
    return elementwise(out, x_t, eps, nullptr, sqrt_recip, neg.data(), nullptr, B, per, stream);
}
extern "C" int dsg_posterior_step(float* out, const float* x_start, const float* x_t, const float* noise,
                                  const float* coef1, const float* coef2, const float* sigma_nz, int B, int64_t per,
                                  void* stream) {
    return elementwise(out, x_start, x_t, noise, coef1, coef2, sigma_nz, B, per, stream);
}
extern "C" int dsg_ddim_step(float* out, const float* x_start, const float* x_t, const float* noise, const float* coef,
                             int B, int64_t per, void* stream) {
    if (!out || !x_start || !x_t || !coef || B <= 0 || per <= 0) return fail(DSG_E_INVALID, "ddim_step: bad argument");
    if (!is_device_ptr(out) || !is_device_ptr(x_start) || !is_device_ptr(x_t) || (noise && !is_device_ptr(noise)))
        return fail(DSG_E_INVALID, "elementwise kernels take device tensors");
    float* dc = nullptr;
    HIPCHK(hipMalloc((void**)&dc, 5 * B * sizeof(float)));
    HIPCHK(hipMemcpy(dc, coef, 5 * B * sizeof(float), hipMemcpyHostToDevice));
    const size_t n = (size_t)B * per;
    hipLaunchKernelGGL(k_ddim_step, dim3((int)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                       out, x_start, x_t, noise, dc, B, (size_t)per);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipFree(dc));
    return 0;
}
