"""ctypes binding of libdsg_hip.so (C ABI: include/dsg.h).

The product path has exactly one backend: the HIP library built in-tree by `make` / `__graft_entry__.build()`.
If it is missing or fails to load, importing a model raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libdsg_hip.so")

E_INVALID, E_RUNTIME, E_UNEXPECTED_KEY, E_MISSING_KEY, E_NOT_IMPLEMENTED, E_STATE = -1, -2, -3, -4, -5, -6
PREC_FP32, PREC_BF16, PREC_BF16W2 = 0, 1, 2
MODE_DDPM, MODE_DDIM = 0, 1
KERNEL_SETS = {"auto": 0, "latency": 1, "tile": 2, "block": 3, "stream": 4, "rows": 5}          # DSG_KSET_* of include/dsg.h
KERNEL_SET_NAMES = {v: k for k, v in KERNEL_SETS.items()}


class dsg_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "variant", "njoints", "n_poses", "n_seed", "latent_dim", "audio_src_dim", "audio_dim", "style_dim_in",
        "window", "num_layers", "num_heads", "ff_size", "local_heads", "pe_max_len", "train_steps", "max_batch",
        "precision", "device", "steps_per_graph", "latency_mode")] + [("reserved", C.c_int32 * 4)]


class dsg_sample_args(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("skip_timesteps", C.c_int32), ("eta", C.c_float), ("const_noise", C.c_int32),
        ("init_noise", C.c_void_p), ("step_noise", C.c_void_p), ("init_image", C.c_void_p),
        ("seed", C.c_uint64), ("stream_id", C.c_uint64), ("draw_base", C.c_uint32), ("n_dump", C.c_int32),
        ("dump_steps", C.c_void_p), ("dump_out", C.c_void_p), ("clip_denoised", C.c_int32), ("first_step", C.c_int32), ("max_steps", C.c_int32), ("reserved", C.c_int32 * 1)]


class dsg_clip_job(C.Structure):
    """One clip of dsg_sample_clip_queue (include/dsg.h)."""
    _fields_ = [
        ("style", C.c_void_p), ("seed0", C.c_void_p), ("seed_last", C.c_void_p), ("audio", C.c_void_p), ("out", C.c_void_p),
        ("K", C.c_int32), ("scale", C.c_float), ("seed", C.c_uint64), ("stream_id", C.c_uint64), ("reserved", C.c_int32 * 4)]


class dsg_clip_edit(C.Structure):
    """The edits of one clip of dsg_sample_clip_queue_edit (include/dsg.h): parallel to the jobs, every pointer nullable."""
    _fields_ = [("inp_mask", C.c_void_p), ("inp_motion", C.c_void_p), ("init_motion", C.c_void_p), ("reserved", C.c_int32 * 2)]


class dsg_queue_job_info(C.Structure):
    """The state of one ticket of a queue session (dsg_queue_job, include/dsg.h)."""
    _fields_ = [("state", C.c_int32), ("windows_done", C.c_int32), ("rows_ready", C.c_int32), ("slot", C.c_int32), ("first_round", C.c_int32),
                ("reserved", C.c_int32 * 3)]


JOB_PENDING, JOB_RUNNING, JOB_DONE, JOB_CANCELLED = 0, 1, 2, 3          # DSG_JOB_* of include/dsg.h
JOB_LIVE, JOB_FINISHED = 1, 2          # bits of dsg_queue_job_info.live (reserved[1] here; reserved[0]: windows_given)
JOB_PARKED = 4                         # DSG_JOB_PARKED: a job that left its slot at a window boundary (reserved[2] here: parks)
JOB_HELD = 4                           # DSG_JOB_HELD, a bit of .live: the caller asked the job to wait (dsg_queue_park)


class dsg_queue_window(C.Structure):
    """One window of dsg_queue_append (include/dsg.h): its audio, and optionally the style / scale from this window on."""
    _fields_ = [("audio", C.c_void_p), ("style", C.c_void_p), ("scale", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


WIN_SCALE, WIN_LAST = 1, 2          # DSG_WIN_* of include/dsg.h

# every symbol include/dsg.h declares: name -> (restype, argtypes)
_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
SYMBOLS = {
    "dsg_version": (_I, []),
    "dsg_last_error": (C.c_char_p, []),
    "dsg_create": (_I, [C.POINTER(dsg_config), C.POINTER(_P)]),
    "dsg_clone": (_I, [_P, _I, C.POINTER(_P)]),
    "dsg_destroy": (_I, [_P]),
    "dsg_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "dsg_finalize_weights": (_I, [_P]),
    "dsg_set_schedule": (_I, [_P, _P, _P, _I]),
    "dsg_schedule_tables": (_I, [_P, _I, _P]),
    "dsg_set_seed_last": (_I, [_P, _P, _I, _P]),
    "dsg_set_window_cond": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dsg_set_window_cond_cfg": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "dsg_set_inpainting": (_I, [_P, _P, _P, _I, _P]),
    "dsg_forward": (_I, [_P, _P, _P, _P, _I, _P]),
    "dsg_sample": (_I, [_P, C.POINTER(dsg_sample_args), _P, _I, _P]),
    "dsg_sample_multi": (_I, [C.POINTER(_P), _I, C.POINTER(dsg_sample_args), C.POINTER(_P), _I, _P]),
    "dsg_set_clip_inpainting": (_I, [_P, _P, _P, _I, _I, _P]),
    "dsg_set_clip_init": (_I, [_P, _P, _I, _I, _P]),
    "dsg_set_noise_streams": (_I, [_P, _P, _P, _I]),
    "dsg_sample_clip": (_I, [_P, _P, _P, _P, _P, _I, _P, C.POINTER(dsg_sample_args), _I, _I, _I, _P, _I, _P]),
    "dsg_sample_clip_multi": (_I, [C.POINTER(_P), _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P, _I, C.POINTER(_P),
                                   C.POINTER(dsg_sample_args), _I, _I, _I, C.POINTER(_P), _I, _P]),
    "dsg_clip_queue_plan": (_I, [_P, _I, _I, _P, _P, C.POINTER(C.c_int32)]),
    "dsg_sample_clip_queue": (_I, [C.POINTER(_P), _I, C.POINTER(dsg_clip_job), _I, _I, _P, _I, C.POINTER(dsg_sample_args), _I, _I, _P]),
    "dsg_sample_clip_queue_edit": (_I, [C.POINTER(_P), _I, C.POINTER(dsg_clip_job), C.POINTER(dsg_clip_edit), _I, _I, _P, _I,
                                        C.POINTER(dsg_sample_args), _I, _I, _P]),
    "dsg_sample_clip_queue_steps": (_I, [C.POINTER(_P), _I, C.POINTER(dsg_clip_job), C.POINTER(dsg_clip_edit), _P, _I, _I, _P, _I,
                                         C.POINTER(dsg_sample_args), _I, _I, _P]),
    "dsg_clip_queue_plan_steps": (_I, [_P, _P, _I, _I, _P, _P, C.POINTER(C.c_int32), C.POINTER(_I64)]),
    "dsg_queue_open": (_I, [C.POINTER(_P), _I, _I, _P, _I, C.POINTER(dsg_sample_args), _I, _I, C.POINTER(_P)]),
    "dsg_queue_submit": (_I, [_P, C.POINTER(dsg_clip_job), C.POINTER(dsg_clip_edit), _I, C.POINTER(_I64), _P]),
    "dsg_queue_run": (_I, [_P, _I, C.POINTER(_I), _P]),
    "dsg_queue_job": (_I, [_P, _I64, C.POINTER(dsg_queue_job_info)]),
    "dsg_queue_info": (_I, [_P, C.POINTER(_I64), C.POINTER(_I), C.POINTER(_I)]),
    "dsg_queue_cancel": (_I, [_P, _I64]),
    "dsg_queue_close": (_I, [_P]),
    "dsg_queue_place": (_I, [_P, _P, _I, _I, _P, _P, C.POINTER(C.c_int32)]),
    "dsg_queue_submit_live": (_I, [_P, C.POINTER(dsg_clip_job), _I, _I, C.POINTER(_I64), _P]),
    "dsg_queue_append": (_I, [_P, _I64, C.POINTER(dsg_queue_window), _I, _P]),
    "dsg_queue_finish": (_I, [_P, _I64]),
    "dsg_queue_set_priority": (_I, [_P, _I64, C.c_int32]),
    "dsg_queue_park": (_I, [_P, _I64]),
    "dsg_queue_resume": (_I, [_P, _I64]),
    "dsg_queue_place_prio": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, C.POINTER(C.c_int32)]),
    "dsg_set_kernel_set": (_I, [_P, _I]),
    "dsg_get_kernel_set": (_I, [_P, C.POINTER(_I)]),
    "dsg_recommend_kernel_set": (_I, [_P, _I, _I, C.POINTER(_I)]),
    "dsg_last_kernel_set": (_I, [_P, C.POINTER(_I)]),
    "dsg_sync": (_I, [_P]),
    "dsg_last_sample_ms": (_I, [_P, C.POINTER(C.c_float), C.POINTER(_I)]),
    "dsg_last_sample_path": (_I, [_P, C.POINTER(_I)]),
    "dsg_last_sample_fence_free": (_I, [_P, C.POINTER(_I)]),
    "dsg_trim": (_I, [_I, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "dsg_noise": (_I, [_P, _I, _I, _I, C.c_uint64, C.c_uint64, C.c_uint32, _P]),
    "dsg_noise_streams": (_I, [_P, _I, _I, _I, _P, _P, C.c_uint32, _P]),
    "dsg_pose2bvh": (_I, [_P, _I, _I, _P, _P, _I, C.c_char_p]),
    "dsg_pose2bvh_channels": (_I, [_P, _I, _I, _P, _P, _I, _P, _P]),
    "dsg_pose2bvh_batch": (_I, [_P, _I, _I, _I, _P, _P, _I, C.POINTER(C.c_char_p)]),
    "dsg_q_sample": (_I, [_P, _P, _P, _P, _P, _I, _I64, _P]),
    "dsg_predict_xstart_from_eps": (_I, [_P, _P, _P, _P, _P, _I, _I64, _P]),
    "dsg_posterior_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, _P]),
    "dsg_ddim_step": (_I, [_P, _P, _P, _P, _P, _I, _I64, _P]),
}


class DSGError(RuntimeError):
    pass


class DSGLibrary:
    def __init__(self, path: str | None = None):
        path = path or os.environ.get("DSG_LIB", DEFAULT_LIB)
        if not os.path.exists(path):
            raise DSGError(
                f"{path} not found: build the HIP library first (`make` or `python -c 'import __graft_entry__ as g; "
                f"g.build()'`).  There is no CPU fallback for the sampling path.")
        self.path = path
        # torch (when installed) must own the HIP runtime of the process: the library exchanges hipStream_t handles and
        # device pointers with it, and a second libamdhip64 initialised first leaves the later one without devices
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.cdll = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(self.cdll, name)          # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        if self.cdll.dsg_version() < 330:
            raise DSGError("libdsg_hip.so is older than this package")

    def check(self, rc: int):
        if rc == 0:
            return
        msg = (self.cdll.dsg_last_error() or b"").decode(errors="replace")
        if rc in (E_INVALID, E_UNEXPECTED_KEY, E_MISSING_KEY):
            raise ValueError(msg)
        if rc == E_NOT_IMPLEMENTED:
            raise NotImplementedError(msg)
        raise DSGError(f"[{rc}] {msg}")


def trim(device: int = -1, library: "DSGLibrary | None" = None):
    """dsg_trim: hand the uncached arenas that hold no live block back to HIP; returns (bytes released, bytes still held)."""
    lib = library or default_library()
    rel, held = C.c_longlong(0), C.c_longlong(0)
    lib.check(lib.cdll.dsg_trim(device, C.byref(rel), C.byref(held)))
    return int(rel.value), int(held.value)


def clip_queue_plan(K, n_slots: int, library: "DSGLibrary | None" = None, n_run=None):
    """dsg_clip_queue_plan: the schedule dsg_sample_clip_queue follows for clips of K[j] windows over n_slots slots (host only).
    Returns (slot[j], first_round[j], n_rounds).  With `n_run` (steps per clip: the schedule length minus the clip's skip_timesteps)
    dsg_clip_queue_plan_steps, the schedule of a queue with per-clip skip_timesteps: returns (slot[j], first_round[j], n_rounds,
    total_steps), total_steps = the sum over the rounds of the deepest clip alive in each."""
    lib = library or default_library()
    k = np.ascontiguousarray(K, dtype=np.int32)
    slot, first, n_rounds = np.zeros(len(k), np.int32), np.zeros(len(k), np.int32), C.c_int32(0)
    if n_run is not None:
        nr = np.ascontiguousarray(n_run, dtype=np.int32)
        if nr.shape != k.shape:
            raise ValueError(f"clip_queue_plan: n_run has {nr.size} entries for {k.size} clips")
        total = C.c_int64(0)
        lib.check(lib.cdll.dsg_clip_queue_plan_steps(k.ctypes.data, nr.ctypes.data, len(k), int(n_slots), slot.ctypes.data, first.ctypes.data,
                                                     C.byref(n_rounds), C.byref(total)))
        return slot.tolist(), first.tolist(), int(n_rounds.value), int(total.value)
    lib.check(lib.cdll.dsg_clip_queue_plan(k.ctypes.data, len(k), int(n_slots), slot.ctypes.data, first.ctypes.data, C.byref(n_rounds)))
    return slot.tolist(), first.tolist(), int(n_rounds.value)


def queue_place(K, n_slots: int, arrive_round=None, library: "DSGLibrary | None" = None):
    """dsg_queue_place: the placement a queue session follows (host only) -- at the start of every round the free slots, lowest first, take
    the pending jobs, oldest ticket first.  `arrive_round[j]`: the session round before which job j is submitted (non-decreasing; None:
    all 0).  Returns (slot[j], first_round[j], n_rounds)."""
    lib = library or default_library()
    k = np.ascontiguousarray(K, dtype=np.int32)
    arr = None if arrive_round is None else np.ascontiguousarray(arrive_round, dtype=np.int32)
    if arr is not None and arr.shape != k.shape:
        raise ValueError(f"queue_place: arrive_round has {arr.size} entries for {k.size} jobs")
    slot, first, n_rounds = np.zeros(len(k), np.int32), np.zeros(len(k), np.int32), C.c_int32(0)
    lib.check(lib.cdll.dsg_queue_place(k.ctypes.data, None if arr is None else arr.ctypes.data, len(k), int(n_slots), slot.ctypes.data,
                                       first.ctypes.data, C.byref(n_rounds)))
    return slot.tolist(), first.tolist(), int(n_rounds.value)


def queue_place_prio(K, n_slots: int, arrive_round=None, priority=None, library: "DSGLibrary | None" = None):
    """dsg_queue_place_prio: the rounds of a queue session with priorities (host only) -- every round the waiting jobs, by priority
    descending then ticket ascending, take the free slots and then the slots of running jobs of a strictly lower priority, which are
    parked.  Returns (first_round[j], done_round[j], n_parks[j], n_rounds); done_round: the round of a job's last window."""
    lib = library or default_library()
    k = np.ascontiguousarray(K, dtype=np.int32)
    opt = {}
    for name, v in (("arrive_round", arrive_round), ("priority", priority)):
        opt[name] = None if v is None else np.ascontiguousarray(v, dtype=np.int32)
        if opt[name] is not None and opt[name].shape != k.shape:
            raise ValueError(f"queue_place_prio: {name} has {opt[name].size} entries for {k.size} jobs")
    arr, pri = opt["arrive_round"], opt["priority"]
    first, done, parks, n_rounds = np.zeros(len(k), np.int32), np.zeros(len(k), np.int32), np.zeros(len(k), np.int32), C.c_int32(0)
    lib.check(lib.cdll.dsg_queue_place_prio(k.ctypes.data, None if arr is None else arr.ctypes.data, None if pri is None else pri.ctypes.data,
                                            len(k), int(n_slots), first.ctypes.data, done.ctypes.data, parks.ctypes.data, C.byref(n_rounds)))
    return first.tolist(), done.tolist(), parks.tolist(), int(n_rounds.value)


_default = None


def default_library() -> DSGLibrary:
    global _default
    if _default is None:
        _default = DSGLibrary()
    return _default


# ---- tensor plumbing (torch is only a carrier for device memory; numpy works too) -------------------------------
def is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class Buf:
    """Keeps a contiguous fp32 (or given dtype) view alive and exposes its address."""

    def __init__(self, x, dtype="float32"):
        if x is None:
            self.obj, self.ptr = None, None
            return
        if is_torch(x):
            import torch
            td = {"float32": torch.float32, "int64": torch.int64, "uint8": torch.uint8}[dtype]
            if dtype == "uint8" and x.dtype == torch.bool:
                x = x.to(torch.uint8)
            self.obj = x.detach().to(td).contiguous()
            self.ptr = self.obj.data_ptr()
        else:
            a = np.asarray(x)
            if dtype == "uint8" and a.dtype == np.bool_:
                a = a.astype(np.uint8)
            self.obj = np.ascontiguousarray(a, dtype=dtype)
            self.ptr = self.obj.ctypes.data

    @property
    def p(self):
        return C.c_void_p(self.ptr) if self.ptr is not None else None


def current_stream_ptr(device_index=None):
    """hipStream_t of torch's current stream (0 / None when torch has no GPU)."""
    try:
        import torch
        if torch.cuda.is_available():
            return C.c_void_p(torch.cuda.current_stream(device_index).cuda_stream)
    except Exception:
        pass
    return None
