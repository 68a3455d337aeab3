"""mipgpu -- Python host side of the MI355X-native VVC MIP search engine.

Thin ctypes binding of ``libmipgpu.so`` (C ABI in ``include/mipgpu.h``).  The product
path is the HIP library only: if it is missing this module raises at import of
:class:`MipEngine` -- there is no CPU fallback.

Mirrors the reference's operator surface (main.cpp + main_aux_functions.h):
  * filter names / KernelIdx of the reference whitelist (constants.h:25-34),
  * the per-frame cost table in the reference layout (constants.h:1558-1631),
  * the CSV cost log is written by the C++ CLI (``bin/mipgpu_cli``, main_aux_functions.h:735-798).
"""
from __future__ import annotations

import ctypes
import importlib.util
import os
import sys
import weakref

import numpy as np

from . import layout
from .layout import COSTS_PER_CTU, CUS_PER_CTU, SHAPES, UNAVAILABLE, num_ctus

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MIPGPU_LIB", os.path.join(PKG_DIR, "lib", "libmipgpu.so"))

# Reference whitelist order (constants.h:25-34); index == mip_filter_type.
FILTERS = (
    "filterFrame_1d_int",
    "filterFrame_1d_float",
    "filterFrame_2d_int_quarterCtu",
    "filterFrame_2d_float_quarterCtu",
    "filterFrame_1d_int_5x5",
    "filterFrame_1d_float_5x5",
    "filterFrame_2d_int_5x5_quarterCtu",
    "filterFrame_2d_float_5x5_quarterCtu",
)
FILTER_NONE = -1


class MipError(RuntimeError):
    pass


def filter_index(name) -> int:
    """Filter name (reference spelling) or index -> mip_filter_type; None -> FILTER_NONE."""
    if name is None:
        return FILTER_NONE
    if isinstance(name, (int, np.integer)):
        return int(name)
    if name not in FILTERS:
        raise MipError(f"Filter type {name} not supported")  # main.cpp:74-76
    return FILTERS.index(name)


# mip_pred_item (include/mipgpu.h): one (frame, CU, mode) whose predicted samples are wanted,
# and where they go in the output buffer.
PRED_ITEM = np.dtype([("frame", "<i4"), ("cu", "<i4"), ("mode", "<i4"), ("pitch", "<i4"), ("offset", "<i8")])
PRED_LAYOUTS = {"packed": 0, "frame": 1}   # MIP_PRED_PACKED / MIP_PRED_FRAME
PRED_NONE = 0xFFFF                         # MIP_PRED_NONE: host output samples no item wrote
PART_MAX_LEAVES = 1024                     # MIP_PART_MAX_LEAVES: list entries per CTU of partition_device
PART_MAX_PENALTY = 1 << 20                 # per-shape penalties of the partition decision: 0 .. 1<<20
MODE_PLANAR = 0xF0                         # MIP_MODE_PLANAR / MIP_MODE_DC: best_mode values written by the
MODE_DC = 0xF1                             # merge of intra_device (regular intra modes, not MIP modes)
INTRA_MAX_BIAS = 1 << 20                   # biases of that merge: 0 .. 1<<20
MODE_ANGULAR_BASE = 0x80                   # MIP_MODE_ANGULAR(m) = 0x80 + m: best_mode value of angular mode m (2..66)
ANGULAR_MODES = 65                         # MIP_ANGULAR_MODES: slots of the angular tables, slot = m - 2
ANGULAR_MAX_SEEDS = 3                      # MIP_ANGULAR_MAX_SEEDS: seeds of angular_refine are 1..3
ANGULAR_EVEN_MODES = tuple(range(2, 67, 2))   # the 33 even modes: the usual coarse list of angular_refine
ANG_REFS_SUBSTITUTED = 0                   # MIP_ANG_REFS_SUBSTITUTED: MipEngine.angular_refs, the default
ANG_REFS_EXTENDED = 1                      # MIP_ANG_REFS_EXTENDED: the real above-right / below-left samples
ANG_INTERP_2TAP = 0                        # MIP_ANG_INTERP_2TAP: MipEngine.angular_interp, the default
ANG_INTERP_4TAP = 1                        # MIP_ANG_INTERP_4TAP: VVC's cubic / Gaussian luma interpolation
PRED_REGULAR = 1                           # MIP_PRED_REGULAR: flags bit of predict(..., regular=True)
PRED_ANGULAR = 4                           # MIP_PRED_ANGULAR: flags bit of predict(..., angular=True)
CHAIN_ANGULAR = 1                          # MIP_CHAIN_ANGULAR: flags bit of mip_predicted_frames_ex (the angular stage)
CAND_REGULAR = 1                           # MIP_CAND_REGULAR: flags bit of mip_candidates_frames (Planar / DC are candidates)
CAND_ANGULAR = 2                           # MIP_CAND_ANGULAR: flags bit of mip_candidates_frames (angular modes are candidates)
CAND_MAX_K = 32                            # MIP_CAND_MAX_K: the candidate lists hold 1..32 entries


class _Opts(ctypes.Structure):
    _fields_ = [("filter", ctypes.c_int), ("kernel_idx", ctypes.c_int), ("max_batch", ctypes.c_int),
                ("want_sad_satd", ctypes.c_int), ("slices_per_ctu", ctypes.c_int), ("best_k", ctypes.c_int)]


_lib = None


def _torch_hip_runtime():
    """Path of the HIP runtime bundled in torch's ROCm wheel (torch/lib/libamdhip64.so), or None
    when torch is not installed or bundles none -- found without importing torch."""
    spec = importlib.util.find_spec("torch")
    for d in (spec.submodule_search_locations or []) if spec is not None else []:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            return p
    return None


def _one_hip_runtime():
    """One HIP runtime per process.  torch's ROCm wheel bundles its own libamdhip64 /
    libhsa-runtime64 and loads them by path, so if libmipgpu.so bound /opt/rocm's runtime a
    later `import torch` would bring a second HIP and HSA runtime into the process, and torch
    then finds no GPU once ours has opened it.  So when torch is installed, its bundled
    runtime is loaded first -- by path, with RTLD_GLOBAL, without importing torch (a
    multi-second import with process-wide side effects that numpy-only callers and the CLI
    wrappers do not need) -- and libmipgpu.so binds to it (same soname, libamdhip64.so.7); a
    later `import torch` finds it already mapped.  MIPGPU_NO_TORCH=1 skips this (a process
    that never imports torch: /opt/rocm's runtime)."""
    if "torch" in sys.modules or os.environ.get("MIPGPU_NO_TORCH"):
        return
    path = _torch_hip_runtime()
    if path is not None:
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def hip_runtimes():
    """Paths of the HIP runtime libraries mapped into this process (diagnostic: one expected)."""
    with open("/proc/self/maps") as f:
        return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})


def library():
    """Load libmipgpu.so (raises if it was not built: the HIP path is mandatory)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MipError(f"{LIB_PATH} not found -- build it with `make -C vvc-mip-gpu_amd` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    _one_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    vp, ip, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    sig = {
        "mip_opts_default": (None, [ctypes.POINTER(_Opts)]),
        "mip_engine_create": (ip, [ip, ip, ip, ctypes.POINTER(_Opts), ctypes.POINTER(vp)]),
        "mip_engine_destroy": (ip, [vp]),
        "mip_num_ctus": (ip, [ip, ip]),
        "mip_costs_per_frame": (i64, [ip, ip]),
        "mip_cus_per_frame": (i64, [ip, ip]),
        "mip_shape_name": (ctypes.c_char_p, [ip]),
        "mip_shape_info": (ip, [ip] + [ctypes.POINTER(ip)] * 5),
        "mip_cu_position": (ip, [ip, ip, ctypes.POINTER(ip), ctypes.POINTER(ip)]),
        "mip_filter_frames": (ip, [vp, vp, ip, ip, ip, vp]),
        "mip_search_frames": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp]),
        "mip_search_frames_async": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_uint64)]),
        "mip_wait": (ip, [vp, ctypes.c_uint64]),
        "mip_flush": (ip, [vp]),
        "mip_device_cache": (ip, [ip, ip, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "mip_search_device": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp, vp]),
        "mip_search_device_range": (ip, [vp, vp, vp, ip, ip, ip, vp, vp, vp, vp]),
        "mip_check_input": (ip, [vp, vp]),
        "mip_unavailable_cus": (ip, [ip, ip, ip, vp]),
        "mip_extended_refs": (ip, [ip, ip, ip, vp, vp]),
        "mip_angular_refs": (ip, [vp, ip]),
        "mip_angular_refs_get": (ip, [vp]),
        "mip_angular_interp": (ip, [vp, ip]),
        "mip_angular_interp_get": (ip, [vp]),
        "mip_angular_filter": (ip, [ip, ip, ip]),
        "mip_filter_device": (ip, [vp, vp, ip, ip, ip, ip, ip, vp]),
        "mip_copy_device": (ip, [vp, vp, ctypes.c_size_t, vp]),
        "mip_topk_device": (ip, [vp, ip, ip, ip, ip, vp, vp, vp]),
        "mip_pred_layout": (ip, [ip, ip, ip, ip, vp, i64, ctypes.POINTER(i64)]),
        "mip_predict_device": (ip, [vp, vp, vp, ip, vp, i64, vp, i64, vp, vp]),
        "mip_predict_frames": (ip, [vp, vp, vp, ip, vp, i64, vp, i64, ctypes.POINTER(i64)]),
        "mip_predict_device_ex": (ip, [vp, vp, vp, ip, vp, i64, vp, i64, vp, ctypes.c_uint, vp]),
        "mip_predict_frames_ex": (ip, [vp, vp, vp, ip, vp, i64, vp, i64, ctypes.c_uint, ctypes.POINTER(i64)]),
        "mip_predicted_frames": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mip_predicted_frames_ex": (ip, [vp, vp, vp, ip, vp, vp, vp, ip, ctypes.c_int32, ctypes.c_uint, vp, vp, vp, vp, vp, vp]),
        "mip_partition_device": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp, vp, vp]),
        "mip_partition_frames": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp, vp]),
        "mip_intra_device": (ip, [vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp]),
        "mip_intra_frames": (ip, [vp, vp, vp, ip, vp, vp, vp]),
        "mip_angular_device": (ip, [vp, vp, vp, ip, vp, ip, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp]),
        "mip_angular_frames": (ip, [vp, vp, vp, ip, vp, ip, vp, vp, vp]),
        "mip_angular_refine_device": (ip, [vp, vp, vp, ip, vp, ip, ip, vp, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp]),
        "mip_angular_refine_frames": (ip, [vp, vp, vp, ip, vp, ip, ip, vp, vp, vp, vp]),
        "mip_candidates_device": (ip, [ip, ip, ip, ip, vp, vp, ip, vp, vp, vp, ctypes.c_int32, vp, vp, vp]),
        "mip_candidates_frames": (ip, [vp, vp, vp, ip, ip, ctypes.c_uint, vp, vp, ip, ip, ctypes.c_int32, vp, vp]),
        "mip_time_search_device": (ctypes.c_double, [vp, vp, vp, ip, vp, ip]),
        "mip_host_stats": (ip, [vp, ctypes.POINTER(ctypes.c_uint64), ip]),
        "mip_search_census": (ip, [vp, ctypes.POINTER(ctypes.c_uint64), ip]),
        "mip_host_alloc": (ip, [ctypes.c_size_t, ctypes.POINTER(vp)]),
        "mip_host_free": (ip, [vp]),
        "mip_host_alloc_near": (ip, [ip, ctypes.c_size_t, ctypes.POINTER(vp)]),
        "mip_bind_thread": (ip, [ip]),
        "mip_numa_node": (ip, [ip]),
        "mip_numa_node_of_pci": (ip, [ctypes.c_char_p]),
        "mip_last_error": (ctypes.c_char_p, []),
        "mip_abi_version": (ip, []),
        "mip_build_id": (ctypes.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def build_id() -> str:
    """mip_build_id(): 'src:<source + flag hash> git:<commit>[ knobs:...]'."""
    return library().mip_build_id().decode()


def source_id(bid: str) -> str:
    """The part of a build ID that identifies the compiled code (the 'src:' token)."""
    return bid.split()[0] if bid else ""


def _check(rc):
    if rc != 0:
        raise MipError(library().mip_last_error().decode())


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


def pinned_empty(shape, dtype, device=None) -> np.ndarray:
    """Uninitialised numpy array in page-locked host memory (mip_host_alloc; with `device`,
    mip_host_alloc_near: on that GPU's NUMA node); transfers to / from it run at DMA rate.
    The memory is released with the last view of it."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    p = ctypes.c_void_p()
    if device is None:
        _check(library().mip_host_alloc(max(1, count * dt.itemsize), ctypes.byref(p)))
    else:
        _check(library().mip_host_alloc_near(int(device), max(1, count * dt.itemsize), ctypes.byref(p)))
    buf = (ctypes.c_byte * max(1, count * dt.itemsize)).from_address(p.value)
    weakref.finalize(buf, library().mip_host_free, ctypes.c_void_p(p.value))
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


class _Ticket:
    """An asynchronous host search in flight: its number, its outputs, and its inputs (kept
    alive until the search has completed).  A ticket dropped without wait() waits in its
    finaliser, so numpy never frees arrays the engine's copies may still be using.  The
    finaliser may run on any thread (garbage collection): it takes the engine's lock, like
    every engine call, because mip_wait drains the engine's bounce ring (not thread safe)."""

    def __init__(self, value, out, keep, engine=None):
        self.value, self.out, self._keep, self._engine = value, out, keep, engine
        self.done = engine is None

    def __del__(self):
        eng = getattr(self, "_engine", None)
        if getattr(self, "done", True) or eng is None:
            return
        try:
            with eng._lock:
                if getattr(eng, "_h", None) and library().mip_wait(eng._h, ctypes.c_uint64(self.value)) != 0:
                    # a finaliser cannot raise: a dropped call's error (e.g. the input contract,
                    # reported per call by mip_wait) becomes a warning instead of vanishing
                    import warnings
                    warnings.warn("dropped search ticket %d failed: %s" % (self.value, library().mip_last_error().decode()),
                                  RuntimeWarning, stacklevel=2)
        except Exception:
            pass


class MipEngine:
    """One engine per GPU (mip_engine_create).  Calls on one engine are serialised by a
    per-engine lock (the C engine must be used by one thread at a time); use one engine per
    thread for concurrency."""

    def __init__(self, width: int, height: int, device: int = 0, filter=None, kernel_idx: int = 0,
                 max_batch: int = 1, want_sad_satd: bool = False, slices_per_ctu: int = 0, best_k: int = 1):
        import threading
        self._lock = threading.RLock()
        L = library()
        self.width, self.height = int(width), int(height)
        self.nctus = num_ctus(self.width, self.height)
        self.filter = filter_index(filter)
        self.kernel_idx = int(kernel_idx)
        self.max_batch = int(max_batch)
        self.want_sad_satd = bool(want_sad_satd)
        self.best_k = int(best_k)
        o = _Opts(self.filter, self.kernel_idx, self.max_batch, int(self.want_sad_satd), int(slices_per_ctu),
                  self.best_k)
        h = ctypes.c_void_p()
        _check(L.mip_engine_create(int(device), self.width, self.height, ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        lock = getattr(self, "_lock", None)
        if lock is None:
            return
        with lock:
            if getattr(self, "_h", None):
                library().mip_engine_destroy(self._h)  # synchronises the engine streams first
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def angular_refs(self) -> int:
        """ANG_REFS_SUBSTITUTED (the default) or ANG_REFS_EXTENDED: the reference lines of every
        angular entry point of this engine (mip_angular_refs).  A call uses the setting it finds when
        it is made; work already enqueued keeps its own."""
        with self._lock:
            value = library().mip_angular_refs_get(self._h)
            _check(min(value, 0))
            return value

    @angular_refs.setter
    def angular_refs(self, value):
        with self._lock:
            _check(library().mip_angular_refs(self._h, int(value)))

    @property
    def angular_interp(self) -> int:
        """ANG_INTERP_2TAP (the default) or ANG_INTERP_4TAP: the interpolation filter of every angular
        entry point of this engine (mip_angular_interp), independent of angular_refs.  A call uses
        the setting it finds when it is made; work already enqueued keeps its own."""
        with self._lock:
            value = library().mip_angular_interp_get(self._h)
            _check(min(value, 0))
            return value

    @angular_interp.setter
    def angular_interp(self, value):
        with self._lock:
            _check(library().mip_angular_interp(self._h, int(value)))

    @property
    def costs_per_frame(self) -> int:
        return self.nctus * COSTS_PER_CTU

    @property
    def cus_per_frame(self) -> int:
        return self.nctus * CUS_PER_CTU

    # ---------------------------------------------------------------- host API
    def _frames(self, frames):
        f = np.ascontiguousarray(frames, dtype=np.uint16)
        if f.ndim == 2:
            f = f[None]
        if f.shape[1:] != (self.height, self.width):
            raise MipError(f"frames of shape {f.shape[1:]} do not match {self.height}x{self.width}")
        return f

    def search(self, frames, refs=None, costs=True, best=False, sad_satd=False, out=None):
        """Full MIP search of host frames ([F,H,W] or [H,W] uint16).  Returns a dict with
        'cost' [F, nCTUs*97840] int32 and optionally 'best_mode' / 'best_cost' [F, nCTUs*5380]
        (decision lists [F, nCTUs*5380, K] when the engine has best_k = K > 1), 'sad' / 'satd'.
        `out` may supply any of these arrays (e.g. from pinned_empty, for DMA-rate
        transfers); the others are allocated."""
        f, r, n, res = self._prepare(frames, refs, costs, best, sad_satd, out)
        with self._lock:  # mip_search_frames: one synchronous call (its last chunks may ramp down)
            _check(library().mip_search_frames(self._h, _ptr(f), _ptr(r), n, _ptr(res.get("cost")),
                                               _ptr(res.get("best_mode")), _ptr(res.get("best_cost")),
                                               _ptr(res.get("sad")), _ptr(res.get("satd"))))
        return res

    def search_async(self, frames, refs=None, costs=True, best=False, sad_satd=False, out=None):
        """As search(), without waiting (mip_search_frames_async): the call queues behind
        the calls in flight and returns a ticket; wait(ticket) returns the output dict.  The
        ticket keeps the input and output arrays alive until then."""
        f, r, n, res = self._prepare(frames, refs, costs, best, sad_satd, out)
        t = ctypes.c_uint64()
        with self._lock:
            _check(library().mip_search_frames_async(self._h, _ptr(f), _ptr(r), n, _ptr(res.get("cost")),
                                                     _ptr(res.get("best_mode")), _ptr(res.get("best_cost")),
                                                     _ptr(res.get("sad")), _ptr(res.get("satd")), ctypes.byref(t)))
        return _Ticket(t.value, res, (f, r), self)

    def _prepare(self, frames, refs, costs, best, sad_satd, out):
        """Input arrays and the output dict of a host search (allocated unless in `out`)."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        given = dict(out or {})

        def buf(key, want, cols, dtype):
            if not want:
                return None
            shape = (n,) + (cols if isinstance(cols, tuple) else (cols,))
            a = given.get(key)
            if a is None:
                return np.empty(shape, dtype)
            if a.dtype != np.dtype(dtype) or a.shape != shape or not a.flags.c_contiguous:
                raise MipError(f"out[{key!r}] must be a C-contiguous {np.dtype(dtype)} array of shape {shape}")
            return a

        res = {}
        bcols = self.cus_per_frame if self.best_k == 1 else (self.cus_per_frame, self.best_k)
        for key, want, cols, dt in (("cost", costs, self.costs_per_frame, np.int32),
                                    ("best_mode", best, bcols, np.uint8), ("best_cost", best, bcols, np.int32),
                                    ("sad", sad_satd, self.costs_per_frame, np.int32),
                                    ("satd", sad_satd, self.costs_per_frame, np.int32)):
            a = buf(key, want, cols, dt)
            if a is not None:
                res[key] = a
        return f, r, n, res

    def wait(self, ticket):
        """Block until an asynchronous search has completed; returns its output dict."""
        with self._lock:
            ticket.done = True  # also on error: the call is over either way
            _check(library().mip_wait(self._h, ctypes.c_uint64(ticket.value)))
        return ticket.out

    def host_stats(self) -> dict:
        """Host-pipeline counters (mip_host_stats): calls, search launches, calls that went
        through merged launches, merged launches."""
        out = (ctypes.c_uint64 * 4)()
        with self._lock:
            _check(library().mip_host_stats(self._h, out, 4))
        return dict(zip(("calls", "launches", "merged_calls", "merged_launches"), (int(v) for v in out)))

    def search_census(self) -> dict:
        """Search launches of the engine so far by kernel instance (mip_search_census): keys
        (waves per workgroup, alt, dec, pf) -- 12, 16 or 8 waves; alternative references;
        decisions only; the prefetching instance -- for all 24 combinations, plus the launch
        counts 'pair' (pair mode), 'chunked' (per-XCD queue chunks) and 'ordered' (items
        longest first)."""
        out = (ctypes.c_uint64 * 27)()
        with self._lock:
            _check(library().mip_search_census(self._h, out, 27))
        res = {(w, a, d, p): int(out[8 * i + 4 * a + 2 * d + p])
               for i, w in enumerate((12, 16, 8)) for a in (0, 1) for d in (0, 1) for p in (0, 1)}
        res.update(pair=int(out[24]), chunked=int(out[25]), ordered=int(out[26]))
        return res

    def flush(self):
        """Launch the engine's open (merged) chunk now (mip_flush): queued small calls are
        otherwise launched by the next call, a wait, or when the chunk is full."""
        with self._lock:
            _check(library().mip_flush(self._h))

    def filter_frames(self, frames, filter, kernel_idx=0):
        f = self._frames(frames)
        out = np.empty_like(f)
        with self._lock:
            _check(library().mip_filter_frames(self._h, _ptr(f), f.shape[0], filter_index(filter), int(kernel_idx),
                                               _ptr(out)))
        return out

    # -------------------------------------------------------------- device API
    def search_device(self, frames, refs=None, costs=None, sad=None, satd=None, best_mode=None,
                      best_cost=None, stream=None):
        """Asynchronous search on device tensors (torch, int16/uint16 [F,H,W]) on `stream`
        (a torch.cuda.Stream; default: torch's current stream).  costs=False: decisions only
        (no cost table; needs best_cost, best_k = 1; returns None)."""
        import torch
        n = frames.shape[0]
        if costs is False:
            costs = None
        elif costs is None:
            costs = torch.empty((n, self.costs_per_frame), dtype=torch.int32, device=frames.device)
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        with self._lock:
            _check(library().mip_search_device(self._h, _ptr(frames), _ptr(refs), n, _ptr(costs), _ptr(sad),
                                               _ptr(satd), _ptr(best_mode), _ptr(best_cost),
                                               ctypes.c_void_p(s.cuda_stream)))
        return costs

    def search_device_range(self, frames, ctu_begin, ctu_end, costs, refs=None, sad=None, satd=None, stream=None):
        """search_device over the CTUs [ctu_begin, ctu_end) of every frame only
        (mip_search_device_range): their blocks of the full-size `costs` are written."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        with self._lock:
            _check(library().mip_search_device_range(self._h, _ptr(frames), _ptr(refs), frames.shape[0],
                                                     int(ctu_begin), int(ctu_end), _ptr(costs), _ptr(sad), _ptr(satd),
                                                     ctypes.c_void_p(s.cuda_stream)))
        return costs

    def check_input(self, stream=None):
        """Input contract of the device-API searches on `stream` (mip_check_input): waits for
        the stream and raises MipError if a search staged a sample above 1023 (10 bits)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        with self._lock:
            _check(library().mip_check_input(self._h, ctypes.c_void_p(s.cuda_stream)))

    # ------------------------------------------------------- prediction output
    def predict(self, frames, items, out_samples, refs=None, regular=False, angular=False):
        """Predicted samples of the list `items` (PRED_ITEM array, see pred_items) for host
        frames (mip_predict_frames).  Returns (uint16 array of out_samples, skipped): samples
        no item wrote are PRED_NONE; skipped counts the items that were not written
        (unavailable CUs, mode "none", blocks that do not fit).  regular=True
        (mip_predict_frames_ex, MIP_PRED_REGULAR): items with mode MODE_PLANAR / MODE_DC are
        emitted too -- the Planar / DC blocks whose costs intra() reports.  angular=True
        (MIP_PRED_ANGULAR): items with mode MODE_ANGULAR_BASE + m, m in 2..66, are emitted too --
        the blocks whose costs angular() reports."""
        flags = (PRED_REGULAR if regular else 0) | (PRED_ANGULAR if angular else 0)
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        it = np.ascontiguousarray(items, dtype=PRED_ITEM)
        out = np.empty(int(out_samples), np.uint16)
        skipped = ctypes.c_int64()
        with self._lock:
            if flags:
                _check(library().mip_predict_frames_ex(self._h, _ptr(f), _ptr(r), f.shape[0], _ptr(it), it.size, _ptr(out),
                                                       int(out_samples), flags, ctypes.byref(skipped)))
            else:
                _check(library().mip_predict_frames(self._h, _ptr(f), _ptr(r), f.shape[0], _ptr(it), it.size, _ptr(out),
                                                    int(out_samples), ctypes.byref(skipped)))
        return out, int(skipped.value)

    def predict_device(self, frames, items, out, refs=None, skipped=None, stream=None, regular=False, angular=False):
        """Asynchronous prediction on device tensors (mip_predict_device): `items` is a uint8
        tensor of the PRED_ITEM bytes (torch.from_numpy(items.view(np.uint8)).cuda()), `out` a
        uint16 / int16 tensor the blocks are written into (other samples are left as they are),
        `skipped` an optional zeroed int32 tensor of one element that counts the items not
        written (final when the call's work on the stream has completed).  regular=True (mip_predict_device_ex, MIP_PRED_REGULAR): items with mode
        MODE_PLANAR / MODE_DC are emitted too, so the item list of partition_device on merged
        decisions gives whole predicted frames.  angular=True (MIP_PRED_ANGULAR): items with an
        angular mode code are emitted too, by a second kernel behind the first.  Returns `out`."""
        import torch
        flags = (PRED_REGULAR if regular else 0) | (PRED_ANGULAR if angular else 0)
        nbytes = items.numel() * items.element_size()
        if nbytes % PRED_ITEM.itemsize:
            raise MipError("predict_device: items is not a whole number of %d-byte entries" % PRED_ITEM.itemsize)
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        with self._lock:
            if flags:
                _check(library().mip_predict_device_ex(self._h, _ptr(frames), _ptr(refs), frames.shape[0], _ptr(items),
                                                       nbytes // PRED_ITEM.itemsize, _ptr(out), out.numel(), _ptr(skipped),
                                                       flags, ctypes.c_void_p(s.cuda_stream)))
            else:
                _check(library().mip_predict_device(self._h, _ptr(frames), _ptr(refs), frames.shape[0], _ptr(items),
                                                    nbytes // PRED_ITEM.itemsize, _ptr(out), out.numel(), _ptr(skipped),
                                                    ctypes.c_void_p(s.cuda_stream)))
        return out

    def predicted_frames(self, frames, penalty=None, bias=None, refs=None) -> dict:
        """The whole chain on host frames (mip_predicted_frames; needs best_k = 1): decisions,
        Planar / DC merge with `bias` (see intra_device), CTU partition with `penalty` (see
        partition_device) and the partition's predicted frames.  dict of numpy arrays: 'best_mode'
        uint8 / 'best_cost' int32 (the merged decisions) / 'leaf' uint8 [F, nCTUs*5380], 'ctu_cost'
        / 'ctu_leaves' int32 [F, nCTUs] and 'pred' uint16 [F, H, W] -- every leaf's MIP, Planar or
        DC block at its place, PRED_NONE where no leaf is (CTUs without a partition)."""
        return self.predicted_frames_ex(frames, penalty=penalty, bias=bias, refs=refs)

    def predicted_frames_ex(self, frames, penalty=None, bias=None, refs=None, angular=None, angular_bias=0) -> dict:
        """predicted_frames with an optional angular stage (mip_predicted_frames_ex).  angular=None:
        exactly predicted_frames (mip_predicted_frames is called).  angular="all" or a list of
        strictly increasing VVC mode numbers in 2..66: the merge of angular_device over that list
        with `angular_bias` (0 .. 1<<20) runs between the Planar / DC merge and the partition, and
        the prediction emits the angular leaves too -- 'best_mode' / 'best_cost' are the decisions
        after both merges, 'pred' holds every leaf's MIP, Planar, DC or angular block."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        pen, b = _penalty(penalty), _bias(bias)
        if angular is not None:
            if isinstance(angular, str) and angular != "all":
                raise MipError('angular must be None, "all" or a list of modes')
            m = None if isinstance(angular, str) else _modes(angular)
            if int(angular_bias) != np.clip(int(angular_bias), -(1 << 31), (1 << 31) - 1):
                raise MipError("bias does not fit int32")
        res = {"best_mode": np.empty((n, self.cus_per_frame), np.uint8),
               "best_cost": np.empty((n, self.cus_per_frame), np.int32),
               "leaf": np.empty((n, self.cus_per_frame), np.uint8),
               "ctu_cost": np.empty((n, self.nctus), np.int32),
               "ctu_leaves": np.empty((n, self.nctus), np.int32),
               "pred": np.empty((n, self.height, self.width), np.uint16)}
        with self._lock:
            if angular is None:
                _check(library().mip_predicted_frames(self._h, _ptr(f), _ptr(r), n, _ptr(pen), _ptr(b), _ptr(res["best_mode"]),
                                                      _ptr(res["best_cost"]), _ptr(res["leaf"]), _ptr(res["ctu_cost"]),
                                                      _ptr(res["ctu_leaves"]), _ptr(res["pred"])))
            else:
                _check(library().mip_predicted_frames_ex(self._h, _ptr(f), _ptr(r), n, _ptr(pen), _ptr(b), _ptr(m),
                                                         0 if m is None else m.size, int(angular_bias), CHAIN_ANGULAR,
                                                         _ptr(res["best_mode"]), _ptr(res["best_cost"]), _ptr(res["leaf"]),
                                                         _ptr(res["ctu_cost"]), _ptr(res["ctu_leaves"]), _ptr(res["pred"])))
        return res

    # ------------------------------------------------------- partition decision
    def partition(self, frames, penalty=None, refs=None) -> dict:
        """Decisions and CTU partition of host frames (mip_partition_frames; needs best_k = 1):
        dict of numpy arrays 'best_mode' uint8 / 'best_cost' int32 / 'leaf' uint8 [F, nCTUs*5380]
        and 'ctu_cost' / 'ctu_leaves' int32 [F, nCTUs].  `penalty`: see partition_device."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        pen = _penalty(penalty)
        res = {"best_mode": np.empty((n, self.cus_per_frame), np.uint8),
               "best_cost": np.empty((n, self.cus_per_frame), np.int32),
               "leaf": np.empty((n, self.cus_per_frame), np.uint8),
               "ctu_cost": np.empty((n, self.nctus), np.int32),
               "ctu_leaves": np.empty((n, self.nctus), np.int32)}
        with self._lock:
            _check(library().mip_partition_frames(self._h, _ptr(f), _ptr(r), n, _ptr(pen), _ptr(res["best_mode"]),
                                                  _ptr(res["best_cost"]), _ptr(res["leaf"]), _ptr(res["ctu_cost"]),
                                                  _ptr(res["ctu_leaves"])))
        return res

    # ------------------------------------------- Planar / DC baseline costs
    def intra(self, frames, refs=None, sad_satd=False) -> dict:
        """Planar / DC baseline costs of host frames (mip_intra_frames, contract in
        include/mipgpu.h): dict of numpy int32 arrays [F, nCTUs*5380, 2] -- 'cost' (slot 0 Planar,
        slot 1 DC; UNAVAILABLE for unavailable CUs) and, with sad_satd, 'sad' / 'satd'."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        res = {k: np.empty((n, self.cus_per_frame, 2), np.int32) for k in (("cost", "sad", "satd") if sad_satd else ("cost",))}
        with self._lock:
            _check(library().mip_intra_frames(self._h, _ptr(f), _ptr(r), n, _ptr(res["cost"]), _ptr(res.get("sad")),
                                              _ptr(res.get("satd"))))
        return res

    def intra_device(self, frames, cost=None, sad=None, satd=None, refs=None, bias=None, best_mode=None, best_cost=None,
                     stream=None):
        """Asynchronous Planar / DC baseline costs and decision merge on device tensors
        (mip_intra_device): `cost` / `sad` / `satd` int32 [F, nCTUs*5380, 2], each optional;
        `best_mode` uint8 / `best_cost` int32 [F, nCTUs*5380] (given together) hold the K = 1 MIP
        decisions of search_device and are merged in place -- a CU whose Planar (DC) cost plus
        bias[0] (bias[1]), 0 .. 1<<20, is strictly lower gets MODE_PLANAR (MODE_DC) and that cost.
        When nothing is asked for, `cost` is allocated.  Returns `cost`."""
        import torch
        n = frames.shape[0]
        if cost is None and sad is None and satd is None and best_mode is None and best_cost is None:
            cost = torch.empty((n, self.cus_per_frame, 2), dtype=torch.int32, device=frames.device)
        want = {"cost": (cost, 8), "sad": (sad, 8), "satd": (satd, 8), "best_mode": (best_mode, 1), "best_cost": (best_cost, 4)}
        for name, (t, size) in want.items():
            if t is not None and (t.numel() * t.element_size() != n * self.cus_per_frame * size or not t.is_contiguous()):
                raise MipError(f"intra_device: {name} must be a contiguous tensor of {n * self.cus_per_frame * size} bytes")
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        with self._lock:
            _check(library().mip_intra_device(self._h, _ptr(frames), _ptr(refs), n, _ptr(cost), _ptr(sad), _ptr(satd),
                                              _ptr(_bias(bias)), _ptr(best_mode), _ptr(best_cost),
                                              ctypes.c_void_p(s.cuda_stream)))
        return cost

    # ------------------------------------------------- angular intra costs
    def angular(self, frames, refs=None, modes=None, table=False) -> dict:
        """Best angular mode of host frames (mip_angular_frames, contract in include/mipgpu.h)
        over `modes` (strictly increasing VVC mode numbers in 2..66; None: all 65): dict of numpy
        arrays 'ang_mode' uint8 (MODE_ANGULAR_BASE + m; 0xff for unavailable CUs) / 'ang_cost'
        int32 [F, nCTUs*5380] and, with `table`, 'cost' int32 [F, nCTUs*5380, 65] (slot m - 2;
        UNAVAILABLE for modes not in the list and for unavailable CUs)."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        m = _modes(modes)
        res = {"ang_mode": np.empty((n, self.cus_per_frame), np.uint8), "ang_cost": np.empty((n, self.cus_per_frame), np.int32)}
        if table:
            res["cost"] = np.empty((n, self.cus_per_frame, ANGULAR_MODES), np.int32)
        with self._lock:
            _check(library().mip_angular_frames(self._h, _ptr(f), _ptr(r), n, _ptr(m), 0 if m is None else m.size,
                                                _ptr(res.get("cost")), _ptr(res["ang_mode"]), _ptr(res["ang_cost"])))
        return res

    def angular_device(self, frames, modes=None, cost=None, sad=None, satd=None, ang_mode=None, ang_cost=None, refs=None,
                       bias=0, best_mode=None, best_cost=None, stream=None):
        """Asynchronous angular intra costs and decision merge on device tensors
        (mip_angular_device) over `modes` (a host list, see angular): `cost` / `sad` / `satd`
        int32 [F, nCTUs*5380, 65], each optional; `ang_mode` uint8 / `ang_cost` int32
        [F, nCTUs*5380] (given together) receive the best mode of the list and its cost;
        `best_mode` / `best_cost` (given together) hold the K = 1 decisions of search_device, or
        those already merged by intra_device, and are merged in place -- a CU whose best angular
        cost plus `bias` (0 .. 1<<20) is strictly lower gets MODE_ANGULAR_BASE + m and that cost.
        At least one output must be given."""
        import torch
        n = frames.shape[0]
        m = _modes(modes)
        want = {"cost": (cost, 4 * ANGULAR_MODES), "sad": (sad, 4 * ANGULAR_MODES), "satd": (satd, 4 * ANGULAR_MODES),
                "ang_mode": (ang_mode, 1), "ang_cost": (ang_cost, 4), "best_mode": (best_mode, 1), "best_cost": (best_cost, 4)}
        for name, (t, size) in want.items():
            if t is not None and (t.numel() * t.element_size() != n * self.cus_per_frame * size or not t.is_contiguous()):
                raise MipError(f"angular_device: {name} must be a contiguous tensor of {n * self.cus_per_frame * size} bytes")
        if int(bias) != np.clip(int(bias), -(1 << 31), (1 << 31) - 1):
            raise MipError("bias does not fit int32")
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        with self._lock:
            _check(library().mip_angular_device(self._h, _ptr(frames), _ptr(refs), n, _ptr(m), 0 if m is None else m.size,
                                                _ptr(cost), _ptr(sad), _ptr(satd), _ptr(ang_mode), _ptr(ang_cost), int(bias),
                                                _ptr(best_mode), _ptr(best_cost), ctypes.c_void_p(s.cuda_stream)))

    def angular_refine(self, frames, refs=None, modes=None, seeds=1, table=False) -> dict:
        """Coarse-to-fine angular search of host frames (mip_angular_refine_frames): every CU ranks
        `modes` (see angular; the usual coarse list is ANGULAR_EVEN_MODES) and also evaluates the
        +-1 neighbours, inside 2..66 and not in the list, of its own `seeds` (1..3) best modes.
        dict of 'ang_mode' / 'ang_cost' (the best of everything evaluated, ties to the lower mode),
        'tried' uint8 [F, nCTUs*5380] (modes evaluated per CU, 0 for unavailable CUs) and, with
        `table`, 'cost' (slots of modes not evaluated for a CU are UNAVAILABLE)."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        m = _modes(modes)
        res = {"ang_mode": np.empty((n, self.cus_per_frame), np.uint8), "ang_cost": np.empty((n, self.cus_per_frame), np.int32),
               "tried": np.empty((n, self.cus_per_frame), np.uint8)}
        if table:
            res["cost"] = np.empty((n, self.cus_per_frame, ANGULAR_MODES), np.int32)
        with self._lock:
            _check(library().mip_angular_refine_frames(self._h, _ptr(f), _ptr(r), n, _ptr(m), 0 if m is None else m.size, _seeds(seeds),
                                                       _ptr(res.get("cost")), _ptr(res["ang_mode"]), _ptr(res["ang_cost"]),
                                                       _ptr(res["tried"])))
        return res

    def angular_refine_device(self, frames, modes=None, seeds=1, cost=None, sad=None, satd=None, ang_mode=None, ang_cost=None,
                              tried=None, refs=None, bias=0, best_mode=None, best_cost=None, stream=None):
        """Asynchronous coarse-to-fine angular search and decision merge on device tensors
        (mip_angular_refine_device): angular_device's arguments and outputs over the modes each CU
        evaluated -- the list plus the neighbours of its `seeds` best modes, see angular_refine --
        and `tried` uint8 [F, nCTUs*5380], the count of those modes.  At least one output."""
        import torch
        n = frames.shape[0]
        m = _modes(modes)
        want = {"cost": (cost, 4 * ANGULAR_MODES), "sad": (sad, 4 * ANGULAR_MODES), "satd": (satd, 4 * ANGULAR_MODES),
                "ang_mode": (ang_mode, 1), "ang_cost": (ang_cost, 4), "tried": (tried, 1), "best_mode": (best_mode, 1),
                "best_cost": (best_cost, 4)}
        for name, (t, size) in want.items():
            if t is not None and (t.numel() * t.element_size() != n * self.cus_per_frame * size or not t.is_contiguous()):
                raise MipError(f"angular_refine_device: {name} must be a contiguous tensor of {n * self.cus_per_frame * size} bytes")
        if int(bias) != np.clip(int(bias), -(1 << 31), (1 << 31) - 1):
            raise MipError("bias does not fit int32")
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        with self._lock:
            _check(library().mip_angular_refine_device(self._h, _ptr(frames), _ptr(refs), n, _ptr(m), 0 if m is None else m.size,
                                                       _seeds(seeds), _ptr(cost), _ptr(sad), _ptr(satd), _ptr(ang_mode), _ptr(ang_cost),
                                                       _ptr(tried), int(bias), _ptr(best_mode), _ptr(best_cost),
                                                       ctypes.c_void_p(s.cuda_stream)))

    def candidates(self, frames, k=3, regular=True, angular=None, seeds=0, intra_bias=None, angular_bias=0, refs=None) -> dict:
        """K-best candidate lists of host frames over the mode families (mip_candidates_frames): per
        chunk the search with MIP lists of length min(k, 32), with `regular` the Planar / DC table,
        with `angular` -- "all" or a mode list as in angular -- the angular table (`seeds` 0: every
        listed mode; 1..3: angular_refine's coarse-to-fine search), then candidates_device.  dict of
        'modes' uint8 / 'costs' int32 [F, nCTUs*5380, k]: the k lowest (cost + bias, rank) modes of
        every CU, 0xff / UNAVAILABLE past its candidates.  intra_bias (Planar, DC) and angular_bias
        are in 0 .. 1<<20."""
        f = self._frames(frames)
        r = None if refs is None else self._frames(refs)
        n = f.shape[0]
        flags = CAND_REGULAR if regular else 0
        m = None
        if angular is not None:
            flags |= CAND_ANGULAR
            m = None if isinstance(angular, str) and angular == "all" else _modes(angular)
        if int(k) != k or not 1 <= int(k) <= CAND_MAX_K:
            raise MipError("k must be an integer in 1..%d" % CAND_MAX_K)
        if int(angular_bias) != np.clip(int(angular_bias), -(1 << 31), (1 << 31) - 1):
            raise MipError("bias does not fit int32")
        res = {"modes": np.empty((n, self.cus_per_frame, int(k)), np.uint8), "costs": np.empty((n, self.cus_per_frame, int(k)), np.int32)}
        b = _bias(intra_bias)
        with self._lock:
            _check(library().mip_candidates_frames(self._h, _ptr(f), _ptr(r), n, int(k), flags, _ptr(b), _ptr(m),
                                                   0 if m is None else m.size, _seeds(seeds), int(angular_bias), _ptr(res["modes"]),
                                                   _ptr(res["costs"])))
        return res

    def time_search_device(self, frames, costs, refs=None, reps=10) -> float:
        with self._lock:
            ms = library().mip_time_search_device(self._h, _ptr(frames), _ptr(refs), frames.shape[0], _ptr(costs),
                                                  int(reps))
        if ms < 0:
            raise MipError(library().mip_last_error().decode())
        return ms


def device_cache(device=0, release=False) -> dict:
    """The process-wide device block cache (mip_device_cache): bytes parked for `device` by
    destroyed engines and blocks reused so far; release=True frees the parked blocks first."""
    idle, reused = ctypes.c_uint64(), ctypes.c_uint64()
    _check(library().mip_device_cache(int(device), int(bool(release)), ctypes.byref(idle), ctypes.byref(reused)))
    return {"idle_bytes": int(idle.value), "reused_blocks": int(reused.value)}


def numa_node(device) -> int:
    """NUMA node of a GPU (mip_numa_node; -1: unknown or a one-node host)."""
    return int(library().mip_numa_node(int(device)))


def bind_thread(device) -> bool:
    """Run the calling thread on the CPUs of the GPU's NUMA node (mip_bind_thread)."""
    return library().mip_bind_thread(int(device)) == 1


def unavailable_cus(width, height, filter=None) -> np.ndarray:
    """Bool per CU (reference order): the CUs an engine with this filter reports as
    MIP_COST_UNAVAILABLE (mip_unavailable_cus; host only)."""
    n = num_ctus(width, height) * CUS_PER_CTU
    out = np.zeros(n, np.uint8)
    _check(library().mip_unavailable_cus(int(width), int(height), filter_index(filter), out.ctypes.data))
    return out.astype(bool)


def angular_filter(lw, lh, mode):
    """0 (cubic) or 1 (Gaussian): the interpolation table a (1 << lw) x (1 << lh) CU takes for the
    angular mode `mode` with ANG_INTERP_4TAP (mip_angular_filter; host only)."""
    value = library().mip_angular_filter(int(lw), int(lh), int(mode))
    _check(min(value, 0))
    return value


def extended_refs(width, height, filter=None):
    """(top, left) uint8 per CU (reference order): how many real samples extend the CU's top line
    (0..h) and its left line (0..w) with ANG_REFS_EXTENDED, for the availability set of an engine
    with this filter (mip_extended_refs; host only)."""
    n = num_ctus(width, height) * CUS_PER_CTU
    top, left = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    _check(library().mip_extended_refs(int(width), int(height), filter_index(filter), top.ctypes.data, left.ctypes.data))
    return top, left


def pred_items(width, height, frame, cu, mode, layout="packed", nframes=None):
    """Prediction list for (frame, cu, mode) triples (arrays broadcast against each other; cu
    as in the decision lists, mode as in best_mode -- 0xff = none): returns (items, out_samples)
    with pitch / offset filled by mip_pred_layout.  layout "packed": blocks back to back in list
    order, row-major w x h (slice with layout.cu_geometry); "frame": blocks at their place in
    `nframes` frame-shaped canvases (default: the largest frame index + 1)."""
    frame, cu, mode = np.broadcast_arrays(np.asarray(frame, np.int64), np.asarray(cu, np.int64), np.asarray(mode, np.int64))
    items = np.zeros(frame.size, PRED_ITEM)
    items["frame"], items["cu"], items["mode"] = frame.ravel(), cu.ravel(), mode.ravel()
    if nframes is None:
        nframes = int(items["frame"].max()) + 1 if items.size else 1
    if layout not in PRED_LAYOUTS:
        raise MipError(f"unknown prediction layout {layout!r}")
    n = ctypes.c_int64()
    _check(library().mip_pred_layout(int(width), int(height), int(nframes), PRED_LAYOUTS[layout], _ptr(items), items.size,
                                     ctypes.byref(n)))
    return items, int(n.value)


def topk_device(costs, width, height, k, modes=None, costs_k=None, stream=None):
    """Per-CU decision lists of device cost tables (torch int32 [F, nCTUs*97840]):
    returns (modes uint8, costs int32), each [F, nCTUs*5380, k] (mip_topk_device)."""
    import torch
    n = costs.shape[0]
    shape = (n, num_ctus(width, height) * CUS_PER_CTU, int(k))
    if modes is None:
        modes = torch.empty(shape, dtype=torch.uint8, device=costs.device)
    if costs_k is None:
        costs_k = torch.empty(shape, dtype=torch.int32, device=costs.device)
    s = stream if stream is not None else torch.cuda.current_stream(costs.device)
    _check(library().mip_topk_device(_ptr(costs), int(width), int(height), n, int(k), _ptr(modes), _ptr(costs_k),
                                     ctypes.c_void_p(s.cuda_stream)))
    return modes, costs_k


def candidates_device(width, height, k, mip_mode=None, mip_cost=None, intra_cost=None, intra_bias=None, ang_cost=None, ang_bias=0,
                      modes=None, costs=None, stream=None):
    """K-best candidate lists over the mode families on device tensors (mip_candidates_device,
    contract in include/mipgpu.h): the k lowest (cost + bias, rank) modes of every CU among the
    families given -- `mip_mode` uint8 / `mip_cost` int32 [F, nCTUs*5380, kin] (the decision lists
    of a search or of topk_device), `intra_cost` int32 [F, nCTUs*5380, 2] (intra_device's table;
    intra_bias: Planar, DC), `ang_cost` int32 [F, nCTUs*5380, 65] (angular_device's or
    angular_refine_device's table).  `modes` uint8 / `costs` int32 [F, nCTUs*5380, k]: pass a tensor
    to fill it, False to leave that output out, None to have it allocated.  Returns (modes, costs)
    (None for an output left out).  Every tensor's first dimension is F, a MIP tensor's last is
    kin.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    given = [t for t in (mip_mode, mip_cost, intra_cost, ang_cost) if t is not None]
    if not given:
        raise MipError("candidates: no family given")
    if int(k) != k or not 1 <= int(k) <= CAND_MAX_K:
        raise MipError("candidates: k must be 1..%d" % CAND_MAX_K)
    n, ncu, k = given[0].shape[0], num_ctus(width, height) * CUS_PER_CTU, int(k)
    kin = 0 if mip_mode is None and mip_cost is None else (mip_mode if mip_mode is not None else mip_cost).shape[-1]
    if modes is None:
        modes = torch.empty((n, ncu, k), dtype=torch.uint8, device=given[0].device)
    if costs is None:
        costs = torch.empty((n, ncu, k), dtype=torch.int32, device=given[0].device)
    modes = None if modes is False else modes
    costs = None if costs is False else costs
    want = {"mip_mode": (mip_mode, kin), "mip_cost": (mip_cost, kin * 4), "intra_cost": (intra_cost, 8),
            "ang_cost": (ang_cost, ANGULAR_MODES * 4), "modes": (modes, k), "costs": (costs, k * 4)}
    for name, (t, size) in want.items():
        if t is not None and (t.numel() * t.element_size() != n * ncu * size or not t.is_contiguous()):
            raise MipError(f"candidates_device: {name} must be a contiguous tensor of {n * ncu * size} bytes")
    if int(ang_bias) != np.clip(int(ang_bias), -(1 << 31), (1 << 31) - 1):
        raise MipError("bias does not fit int32")
    s = stream if stream is not None else torch.cuda.current_stream(given[0].device)
    b = _bias(intra_bias)
    _check(library().mip_candidates_device(int(width), int(height), n, k, _ptr(mip_mode), _ptr(mip_cost), int(kin), _ptr(intra_cost),
                                           _ptr(b), _ptr(ang_cost), int(ang_bias), _ptr(modes), _ptr(costs),
                                           ctypes.c_void_p(s.cuda_stream)))
    return modes, costs


def _penalty(penalty):
    """Per-shape penalties as the int32 [47] host array of the C ABI (None: zeros): a scalar (the
    same for every shape) or a 47-vector.  The range is checked by the library."""
    if penalty is None:
        return None
    p = np.asarray(penalty)
    if p.ndim == 0:
        p = np.full(len(SHAPES), p)
    if p.shape != (len(SHAPES),):
        raise MipError("penalty must be a scalar or one value per CU shape (%d)" % len(SHAPES))
    if np.any(p != np.clip(p, -(1 << 31), (1 << 31) - 1)):
        raise MipError("penalty does not fit int32")
    return np.ascontiguousarray(p, dtype=np.int32)


def _bias(bias):
    """The merge biases of intra_device as the int32 [2] host array of the C ABI (None: zeros):
    (Planar, DC).  The range is checked by the library."""
    if bias is None:
        return None
    b = np.asarray(bias)
    if b.shape != (2,):
        raise MipError("bias must be two values (Planar, DC)")
    if np.any(b != np.clip(b, -(1 << 31), (1 << 31) - 1)):
        raise MipError("bias does not fit int32")
    return np.ascontiguousarray(b, dtype=np.int32)


def _modes(modes):
    """The mode list of angular / angular_device as the uint8 host array of the C ABI (None: all
    65 modes).  Order and range are checked by the library; an empty list is refused here, since
    the C ABI reads it as "all"."""
    if modes is None:
        return None
    m = np.asarray(modes)
    if m.ndim != 1 or m.size == 0 or m.size > ANGULAR_MODES or np.any(m != np.clip(m, 0, 255)):
        raise MipError("modes must be 1..%d mode numbers in 2..66" % ANGULAR_MODES)
    return np.ascontiguousarray(m, dtype=np.uint8)


def _seeds(seeds):
    """seeds of angular_refine as the C int (the library checks the range 1..ANGULAR_MAX_SEEDS)."""
    if int(seeds) != seeds or int(seeds) != np.clip(int(seeds), -(1 << 31), (1 << 31) - 1):
        raise MipError("seeds must be an integer in 1..%d" % ANGULAR_MAX_SEEDS)
    return int(seeds)


def partition_device(best_cost, width, height, penalty=None, best_mode=None, leaf=None, ctu_cost=None, ctu_leaves=None,
                     items=None, stream=None):
    """CTU partition decision on device tensors (mip_partition_device, contract in
    include/mipgpu.h): `best_cost` int32 [F, nCTUs*5380] (the K = 1 list of a search), `penalty` a
    scalar or 47-vector in 0 .. 1<<20 added per leaf of a shape (the caller's rate term).
    Outputs, each optional, at least one: `leaf` uint8 [F, nCTUs*5380], `ctu_cost` /
    `ctu_leaves` int32 [F, nCTUs], `items` uint8 [F, nCTUs, PART_MAX_LEAVES * 24] (PRED_ITEM
    bytes; needs `best_mode` uint8 [F, nCTUs*5380]) -- a device list for predict_device.
    Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    n = best_cost.shape[0]
    nct = num_ctus(width, height)
    want = {"best_cost": (best_cost, n * nct * CUS_PER_CTU * 4), "best_mode": (best_mode, n * nct * CUS_PER_CTU),
            "leaf": (leaf, n * nct * CUS_PER_CTU), "ctu_cost": (ctu_cost, n * nct * 4), "ctu_leaves": (ctu_leaves, n * nct * 4),
            "items": (items, n * nct * PART_MAX_LEAVES * PRED_ITEM.itemsize)}
    for name, (t, nbytes) in want.items():
        if t is not None and (t.numel() * t.element_size() != nbytes or not t.is_contiguous()):
            raise MipError(f"partition_device: {name} must be a contiguous tensor of {nbytes} bytes")
    s = stream if stream is not None else torch.cuda.current_stream(best_cost.device)
    _check(library().mip_partition_device(_ptr(best_cost), _ptr(best_mode), int(width), int(height), n, _ptr(_penalty(penalty)),
                                          _ptr(leaf), _ptr(ctu_cost), _ptr(ctu_leaves), _ptr(items),
                                          ctypes.c_void_p(s.cuda_stream)))


def copy_device(src, dst, stream=None):
    """Streaming device copy of tensor `src` into `dst` (mip_copy_device; same byte size)."""
    import torch
    n = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != n:
        raise MipError("copy_device: sizes differ")
    s = stream if stream is not None else torch.cuda.current_stream(src.device)
    _check(library().mip_copy_device(_ptr(src), _ptr(dst), n, ctypes.c_void_p(s.cuda_stream)))
    return dst


def filter_device(frames_in, frames_out, filter, kernel_idx=0, stream=None):
    import torch
    n, h, w = frames_in.shape
    s = stream if stream is not None else torch.cuda.current_stream(frames_in.device)
    _check(library().mip_filter_device(_ptr(frames_in), _ptr(frames_out), w, h, n, filter_index(filter),
                                       int(kernel_idx), ctypes.c_void_p(s.cuda_stream)))
    return frames_out


__all__ = ["MODE_PLANAR", "MODE_DC", "INTRA_MAX_BIAS", "MODE_ANGULAR_BASE", "ANGULAR_MODES", "ANGULAR_MAX_SEEDS", "ANGULAR_EVEN_MODES", "ANG_REFS_SUBSTITUTED", "ANG_REFS_EXTENDED", "extended_refs", "ANG_INTERP_2TAP", "ANG_INTERP_4TAP", "angular_filter", "PRED_REGULAR", "PRED_ANGULAR", "CHAIN_ANGULAR", "PRED_ITEM", "PRED_NONE", "pred_items", "PART_MAX_LEAVES", "PART_MAX_PENALTY", "partition_device", "MipEngine", "MipError", "build_id", "source_id", "FILTERS", "FILTER_NONE", "filter_index", "filter_device", "topk_device", "library",
           "pinned_empty", "unavailable_cus", "numa_node", "bind_thread", "device_cache", "copy_device",
           "layout", "SHAPES", "COSTS_PER_CTU", "CUS_PER_CTU", "UNAVAILABLE", "num_ctus"]
