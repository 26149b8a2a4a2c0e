"""ctypes binding of libtangency.so (include/tangency_posterior.h).

This is the ONLY compute path of the package: there is no CPU fallback.  Importing the module loads
the shared library (so that a missing build fails loudly); creating a `Device` needs a gfx950 GPU.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import sys
import threading
import weakref
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TANGENCY_LIB selects another build of the same library (tuning experiments); default: the in-tree one
LIB_PATH = os.environ.get("TANGENCY_LIB") or os.path.join(_HERE, "libtangency.so")

TP_OK = 0
TP_ERR_INVALID = -1
TP_ERR_NO_DEVICE = -2
TP_ERR_HIP = -3
TP_ERR_UNSUPPORTED = -4
TP_ERR_RCCL = -5
STRATEGY_CONJUGATE = 0
STRATEGY_JEFFREYS = 1
STATUS_OK, STATUS_NOT_PD, STATUS_NONFINITE, STATUS_BAD_DENOM = 0, 1, 2, 3
STATUS_NO_CONVERGENCE = 4          # TP_STATUS_NO_CONVERGENCE: `spectral_greyserman`'s eigensolver reached SPECTRAL_MAX_SWEEPS
AUX_STRIDE = 8
FLAG_CENTER_BY_ROWS = 1
FLAG_NO_CENTER = 2
FLAG_NO_SHARED_GRAM = 4
UNIQUE_ID_BYTES = 128
SWEEP_MAX_RHS = 16
ERR_INVALID = -1
REPLAY_SUM_CHECK = 1
REPLAY_BAD_WEIGHTS = 2
REPLAY_METRICS = 5
REPLAY_SRC_RUN, REPLAY_SRC_PRIOR_SWEEP, REPLAY_SRC_SIZE_SWEEP, REPLAY_SRC_WINDOW_SWEEP, REPLAY_SRC_GRID_SWEEP = 0, 1, 2, 3, 4
REPLAY_SRC_SWEEP_FINISH = 5
REPLAY_SRC_SPECTRAL = 6
SPECTRAL_MAX_SWEEPS = 32           # TP_SPECTRAL_MAX_SWEEPS
FINISH_GREYSERMAN, FINISH_JORION = 0, 1
FINISH_DRAWS_PER_WAVE = 16        # TP_FINISH_DRAWS_PER_WAVE: consecutive shifts of one window per wavefront of `sweep_finish`
SUMMARY_STATS = 32
SUMMARY_MAX_COSTS = 64
SUMMARY_OK, SUMMARY_NO_REPLAY, SUMMARY_NONFINITE = 0, 1, 2

# every symbol include/tangency_posterior.h declares (checked by tests/test_cabi_symbols.py)
EXPORTS = [
    "tp_version", "tp_max_assets", "tp_sweep_max_assets", "tp_device_count", "tp_create", "tp_destroy", "tp_set_option", "tp_get_option", "tp_last_error",
    "tp_device_info",
    "tp_log_returns", "tp_batch_create", "tp_batch_upload", "tp_batch_upload_async", "tp_batch_upload_wait",
    "tp_batch_shared_gram_blocks",
    "tp_batch_shared_intraday_blocks",
    "tp_addressing_flags", "tp_batch_addressing",
    "tp_host_alloc", "tp_host_free", "tp_batch_set_rhs", "tp_batch_set_shift", "tp_batch_keep_rhs",
    "tp_batch_download_rhs", "tp_batch_keep_posterior", "tp_batch_download_posterior", "tp_batch_run", "tp_batch_download", "tp_batch_download_S1", "tp_batch_download_matrix",
    "tp_batch_solve_sweep", "tp_batch_solve_sweep_tiled", "tp_batch_download_sweep", "tp_batch_download_sweep_rhs",
    "tp_batch_sweep_finish", "tp_batch_download_sweep_finish",
    "tp_batch_spectral_greyserman", "tp_batch_download_spectral",
    "tp_batch_prior_sweep", "tp_batch_prior_sweep_tiled", "tp_batch_download_prior_sweep",
    "tp_batch_size_sweep", "tp_batch_size_sweep_tiled", "tp_batch_download_size_sweep",
    "tp_batch_window_sweep", "tp_batch_window_sweep_tiled", "tp_batch_download_window_sweep",
    "tp_batch_grid_sweep", "tp_batch_grid_sweep_tiled", "tp_batch_download_grid_sweep",
    "tp_replay_merge_maps", "tp_replay_run", "tp_replay_run_batch", "tp_replay_download",
    "tp_replay_summary", "tp_replay_download_summary",
    "tp_batch_debug_stamps", "tp_batch_destroy", "tp_posterior_batch", "tp_synchronize", "tp_last_timing",
    "tp_region_begin", "tp_region_end", "tp_region_steps", "tp_last_launch", "tp_comm_unique_id", "tp_comm_init", "tp_comm_destroy",
    "tp_comm_count", "tp_comm_init_all", "tp_group_gather",
    "tp_batch_gather", "tp_batch_gather_async", "tp_batch_download_gathered",
]


class TangencyError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libtangency error {code}: {msg}")
        self.code = code


class tp_params_t(ctypes.Structure):
    _fields_ = [("k", c_int32), ("N", c_int32), ("n_r", c_int32), ("m", c_int32), ("strategy", c_int32),
                ("flags", c_int32), ("gamma", c_double)]


class tp_inputs_t(ctypes.Structure):
    _fields_ = [("panel", POINTER(c_double)), ("panel_rows", c_int64), ("panel_ld", c_int32), ("hf_ld", c_int32),
                ("start", POINTER(c_int64)), ("row_idx", POINTER(c_int32)), ("n_rows", POINTER(c_int32)),
                ("col_idx", POINTER(c_int32)), ("rf_adj", POINTER(c_double)),
                ("hf_panel", POINTER(c_double)), ("hf_rows", c_int64),
                ("hf_start", POINTER(c_int64)), ("hf_row_idx", POINTER(c_int32)), ("hf_count", POINTER(c_int32)),
                ("w0", POINTER(c_double)), ("n0", POINTER(c_double)),
                ("ret_num", POINTER(c_int32)), ("ret_den", POINTER(c_int32)), ("ret_rows", c_int64),
                ("hf_ret_num", POINTER(c_int32)), ("hf_ret_den", POINTER(c_int32)), ("hf_ret_rows", c_int64)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C incorporating_different_sources_amd/csrc`.  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.tp_version.restype = c_char_p
    lib.tp_last_error.restype = c_char_p
    lib.tp_last_error.argtypes = [c_void_p]
    lib.tp_max_assets.restype = c_int
    lib.tp_sweep_max_assets.restype = c_int
    lib.tp_create.argtypes = [c_int, POINTER(c_void_p)]
    lib.tp_destroy.argtypes = [c_void_p]
    lib.tp_set_option.argtypes = [c_void_p, c_char_p, c_int]
    lib.tp_get_option.argtypes = [c_void_p, c_char_p, POINTER(c_int)]
    lib.tp_device_info.argtypes = [c_void_p, c_char_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int64)]
    lib.tp_log_returns.argtypes = [c_void_p, POINTER(c_double), c_int64, c_int32, POINTER(c_int32), POINTER(c_int32),
                                   c_int64, POINTER(c_double)]
    lib.tp_batch_create.argtypes = [c_void_p, POINTER(tp_params_t), c_int64, POINTER(c_void_p)]
    lib.tp_batch_upload.argtypes = [c_void_p, POINTER(tp_inputs_t)]
    lib.tp_batch_upload_async.argtypes = [c_void_p, POINTER(tp_inputs_t)]
    lib.tp_batch_upload_wait.argtypes = [c_void_p]
    lib.tp_batch_shared_gram_blocks.argtypes = [c_void_p]
    lib.tp_batch_shared_intraday_blocks.argtypes = [c_void_p]
    lib.tp_addressing_flags.argtypes = [c_int64, c_int32, c_int32]
    lib.tp_batch_addressing.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.tp_host_alloc.argtypes = [POINTER(c_void_p), c_int64]
    lib.tp_host_free.argtypes = [c_void_p]
    lib.tp_batch_keep_rhs.argtypes = [c_void_p, c_int]
    lib.tp_comm_count.argtypes = [c_void_p, POINTER(c_int)]
    lib.tp_comm_init_all.argtypes = [POINTER(c_void_p), c_int]
    lib.tp_group_gather.argtypes = [POINTER(c_void_p), c_int, c_int, POINTER(c_double), POINTER(c_int32)]
    lib.tp_batch_set_rhs.argtypes = [c_void_p, POINTER(c_double)]
    lib.tp_batch_set_shift.argtypes = [c_void_p, POINTER(c_double)]
    lib.tp_batch_download_rhs.argtypes = [c_void_p, POINTER(c_double)]
    lib.tp_batch_keep_posterior.argtypes = [c_void_p, c_int64, c_int64]
    lib.tp_batch_download_posterior.argtypes = [c_void_p, POINTER(c_double)]
    lib.tp_batch_run.argtypes = [c_void_p]
    lib.tp_batch_solve_sweep.argtypes = [c_void_p, c_int32, POINTER(c_double), c_int32, POINTER(c_double), c_int32]
    lib.tp_batch_solve_sweep_tiled.argtypes = [c_void_p, c_int32, POINTER(c_double), c_int32, POINTER(c_double), c_int32]
    lib.tp_batch_download_sweep.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32)]
    lib.tp_batch_download_sweep_rhs.argtypes = [c_void_p, POINTER(c_double)]
    lib.tp_batch_sweep_finish.argtypes = [c_void_p, c_int, c_double, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_download_sweep_finish.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_spectral_greyserman.argtypes = [c_void_p, c_int32, c_double, POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int32]
    lib.tp_batch_download_spectral.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double), POINTER(c_double),
                                               POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_prior_sweep.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_prior_sweep_tiled.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_download_prior_sweep.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_size_sweep.argtypes = [c_void_p, c_int32, POINTER(c_int32), c_int32, POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_size_sweep_tiled.argtypes = [c_void_p, c_int32, POINTER(c_int32), c_int32, POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_download_size_sweep.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_window_sweep.argtypes = [c_void_p, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int32,
                                          POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_window_sweep_tiled.argtypes = lib.tp_batch_window_sweep.argtypes
    lib.tp_batch_download_window_sweep.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_grid_sweep.argtypes = [c_void_p, c_int32, POINTER(c_int32), c_int32, POINTER(c_int32), POINTER(c_int32),
                                        POINTER(c_double), c_int32, POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_grid_sweep_tiled.argtypes = lib.tp_batch_grid_sweep.argtypes
    lib.tp_batch_download_grid_sweep.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_download.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_batch_download_S1.argtypes = [c_void_p, c_int64, POINTER(c_double)]
    lib.tp_batch_download_matrix.argtypes = [c_void_p, c_int64, c_int, POINTER(c_double), POINTER(c_double)]
    lib.tp_batch_debug_stamps.argtypes = [c_void_p, POINTER(c_int64)]
    lib.tp_batch_destroy.argtypes = [c_void_p]
    lib.tp_posterior_batch.argtypes = [c_void_p, POINTER(tp_params_t), c_int64, POINTER(tp_inputs_t),
                                       POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    lib.tp_replay_merge_maps.argtypes = [POINTER(c_int32), c_int64, c_int32, c_int64, c_int32, POINTER(c_int32), POINTER(c_int32)]
    lib.tp_replay_run.argtypes = [c_void_p, c_int64, c_int32, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int32),
                                  c_int32, c_int64, POINTER(c_int32), POINTER(c_double), POINTER(c_double),
                                  POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                  POINTER(c_double), c_int64, POINTER(c_int32), POINTER(c_double), c_int64]
    lib.tp_replay_run_batch.argtypes = [c_void_p, c_int, c_int64, c_int32, POINTER(c_double), POINTER(c_double), c_int64,
                                        POINTER(c_int32), c_int32, c_int64, POINTER(c_int32), POINTER(c_double), POINTER(c_double),
                                        POINTER(c_double), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                        POINTER(c_int64), POINTER(c_int64), POINTER(c_int32), POINTER(c_double), c_int64,
                                        c_int64, POINTER(c_int64), POINTER(c_int32), POINTER(c_double), c_int32]
    lib.tp_replay_download.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32),
                                       POINTER(c_int32)]
    lib.tp_replay_summary.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double)]
    lib.tp_replay_download_summary.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32)]
    lib.tp_synchronize.argtypes = [c_void_p]
    lib.tp_last_timing.argtypes = [c_void_p] + [POINTER(c_double)] * 4
    lib.tp_region_begin.argtypes = [c_void_p]
    lib.tp_region_end.argtypes = [c_void_p, POINTER(c_double)]
    lib.tp_region_steps.argtypes = [c_void_p, POINTER(c_double), c_int, POINTER(c_int)]
    lib.tp_last_launch.argtypes = [c_void_p] + [POINTER(c_int)] * 4
    lib.tp_comm_unique_id.argtypes = [c_void_p]
    lib.tp_comm_init.argtypes = [c_void_p, c_void_p, c_int, c_int]
    lib.tp_comm_destroy.argtypes = [c_void_p]
    lib.tp_batch_gather.argtypes = [c_void_p, c_int, POINTER(c_double), POINTER(c_int32)]
    lib.tp_batch_gather_async.argtypes = [c_void_p, c_int]
    lib.tp_batch_download_gathered.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is not c_char_p:
            fn.restype = c_int
    return lib


lib = _load()


def version() -> str:
    return lib.tp_version().decode()


def max_assets() -> int:
    return int(lib.tp_max_assets())


def sweep_max_assets() -> int:
    """Largest k `Batch.solve_sweep` covers (`tp_sweep_max_assets`)."""
    return int(lib.tp_sweep_max_assets())


def addressing_flags(panel_bytes: int, ld: int, rows_per_window: int) -> int:
    """`tp_addressing_flags`: bit 0 - explicit-row windows, bit 1 - contiguous windows of such a panel load through
    32-bit byte offsets; a clear bit means 64-bit addresses.  Needs no device."""
    return int(lib.tp_addressing_flags(int(panel_bytes), int(ld), int(rows_per_window)))


def replay_merge_maps(cols, K: int):
    """`tp_replay_merge_maps` for a universe table `cols` [R x k] of ticker indices in [0, K): (prev_slot, next_slot), both
    [R x k] - the slot each ticker of date j held at j-1 / holds at j+1, or -1.  Needs no device.  Raises TangencyError
    (TP_ERR_INVALID) for an index outside [0, K) or a ticker twice in one row."""
    if cols is None or np.asarray(cols).dtype.kind not in "iu":
        raise ValueError("cols: an integer array is expected")
    c = np.ascontiguousarray(cols, dtype=np.int32)
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError(f"cols: expected shape (R, k) with R, k >= 1, got {tuple(c.shape)}")
    R, k = c.shape
    prev_slot = np.empty((R, k), dtype=np.int32)
    next_slot = np.empty((R, k), dtype=np.int32)
    rc = lib.tp_replay_merge_maps(_ptr(c, c_int32), R, k, k, int(K), _ptr(prev_slot, c_int32), _ptr(next_slot, c_int32))
    if rc != TP_OK:
        raise TangencyError(rc, lib.tp_last_error(None).decode())
    return prev_slot, next_slot


def device_count() -> int:
    return int(lib.tp_device_count())


def _ptr(a, ct):
    return None if a is None else a.ctypes.data_as(POINTER(ct))


def _arr(a, dtype, shape=None, name=""):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


# ---- lifetime --------------------------------------------------------------------------------------------------------
# Device memory, streams, events and RCCL communicators must be released while the HIP / RCCL runtimes are still up.
# Objects that outlive their scope - locals of a frame kept by a traceback after a failed backtest, module globals -
# used to reach __del__ during interpreter finalisation or never, and the process then aborted in the runtimes' own
# static teardown (round 2: `std::bad_variant_access`, core dumps after a failing test).  Rule: every live Device and
# pinned block is tracked here and closed by ONE atexit hook (atexit hooks run before module teardown and before any
# C-level exit handler: batches first, then the communicator, streams, the handle); finalisers that run once the
# interpreter is finalising do nothing (the library's own exit handler covers whatever is left, see tp_destroy).
_live_devices: "weakref.WeakSet" = weakref.WeakSet()
_live_pinned: "weakref.WeakSet" = weakref.WeakSet()
_live_lock = threading.Lock()
_closed_for_exit = False


def _replay_real(name, a, ndim=None):
    if a is None or np.asarray(a).dtype.kind not in "fiu":
        raise ValueError(f"{name}: a real floating-point array is expected, got dtype {np.asarray(a).dtype}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if ndim is not None and a.ndim != ndim:
        raise ValueError(f"{name}: a {ndim}-D array is expected, got shape {tuple(a.shape)}")
    return a


def _replay_integer(name, a, dtype, shape=None):
    if a is None or np.asarray(a).dtype.kind not in "iu":
        raise ValueError(f"{name}: an integer array is expected")
    wide = np.asarray(a)
    if wide.size and (wide.min() < np.iinfo(dtype).min or wide.max() > np.iinfo(dtype).max):
        raise ValueError(f"{name}: an entry does not fit {np.dtype(dtype).name}")
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and a.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {tuple(a.shape)}")
    return a


def _replay_schedule(S, rf_daily, reb_day, K, k, scaling, cost):
    """The checks `Device.replay` and `Batch.replay` share - returns, risk-free rates, rebalancing days, sizes, scalings and
    costs -: (S, D, ld, K, rf, reb, R, k, P, scaling, cost) as contiguous arrays of the library's types."""
    S = _replay_real("S", S, 2)
    D, ld = S.shape
    if D < 1 or ld < 1:
        raise ValueError(f"S: at least one day and one column expected, got shape {tuple(S.shape)}")
    K = int(K)
    if not 1 <= K <= ld:
        raise ValueError(f"K={K}: within [1, {ld}] (the columns of S) expected")
    rf = _replay_real("rf_daily", rf_daily)
    if rf.shape != (D,):
        raise ValueError(f"rf_daily: expected shape ({D},), got {tuple(rf.shape)}")
    reb = _replay_integer("reb_day", reb_day, np.int32)
    if reb.ndim != 1 or reb.size < 1:
        raise ValueError(f"reb_day: a 1-D array of at least one day is expected, got shape {tuple(reb.shape)}")
    if reb[0] != 0:
        raise ValueError(f"reb_day[0]={int(reb[0])}: the first trading day rebalances")
    if (np.diff(reb) <= 0).any() or reb[-1] >= D:
        raise ValueError(f"reb_day: strictly increasing below D={D} expected")
    R = int(reb.size)
    kk = _replay_integer("k", k, np.int32)
    if kk.ndim != 1:
        raise ValueError(f"k: a 1-D array is expected, got shape {tuple(kk.shape)}")
    P = int(kk.size)
    if P and kk.min() < 1:
        raise ValueError("k: every portfolio holds at least one asset")
    if P and kk.max() > max_assets():
        raise ValueError(f"k={int(kk.max())} exceeds the largest supported universe {max_assets()}")
    sc, co = _replay_real("scaling", scaling), _replay_real("cost", cost)
    for name, a in (("scaling", sc), ("cost", co)):
        if a.shape != (P,):
            raise ValueError(f"{name}: expected shape ({P},), got {tuple(a.shape)}")
    return S, D, ld, K, rf, reb, R, kk, P, sc, co


def _replay_rows_fit(name, off, stride, R, kk, n):
    for p in range(kk.size):
        o, s = int(off[p]), int(stride[p])          # (Python integers: no overflow)
        if o < 0 or s < 0 or o + (R - 1) * s + int(kk[p]) > n:
            raise ValueError(f"{name}_off[{p}]={o}, {name}_stride[{p}]={s}: {R} rows of {int(kk[p])} run past the buffer's "
                             f"{n} elements")


def _finalizing() -> bool:
    return _closed_for_exit or sys.is_finalizing()


def shutdown() -> None:
    """Close every live Device (its batches first) and free every pinned block.  Runs at interpreter exit; safe to
    call earlier (objects created afterwards are tracked again)."""
    with _live_lock:
        devices = list(_live_devices)
        pinned = list(_live_pinned)
    for d in devices:
        try:
            d.close()
        except Exception:
            pass
    for p in pinned:
        try:
            p.free()
        except Exception:
            pass
    global _default_device, _default_group
    _default_device = None
    _default_group = None


def _shutdown_at_exit() -> None:
    global _closed_for_exit
    try:
        shutdown()
    finally:
        _closed_for_exit = True


atexit.register(_shutdown_at_exit)


class _PinnedBlock:
    """Owner of one tp_host_alloc block; numpy arrays made over it keep it alive through `.base`."""

    def __init__(self, nbytes: int):
        self.ptr = c_void_p()
        rc = lib.tp_host_alloc(ctypes.byref(self.ptr), int(nbytes))
        if rc != TP_OK:
            raise TangencyError(rc, f"tp_host_alloc({nbytes}) failed")
        self.nbytes = int(nbytes)
        self.buf = (ctypes.c_char * max(1, self.nbytes)).from_address(self.ptr.value)
        with _live_lock:
            _live_pinned.add(self)

    def free(self):
        if self.ptr:
            lib.tp_host_free(self.ptr)
            self.ptr = c_void_p()

    def __del__(self):
        if _finalizing():        # the runtime may be unloading: leak (the process is ending)
            return
        try:
            self.free()
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64) -> np.ndarray:
    """An uninitialised array in page-locked host memory (`tp_host_alloc`): uploads from it and downloads into it
    run at PCIe rate and, with `Batch.upload_async`, without blocking the host."""
    dtype = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    n = int(np.prod(shape)) if shape else 1
    block = _PinnedBlock(n * dtype.itemsize)
    arr = np.frombuffer(block.buf, dtype=dtype, count=n).reshape(shape)
    # np.frombuffer keeps `block.buf` (and through a reference cycle-free attribute the block) alive
    block.buf._owner = block
    return arr


def pinned_copy(a) -> np.ndarray:
    a = np.asarray(a)
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class Device:
    """One GPU (`tp_handle_t`): a HIP stream, timing events and optionally an RCCL communicator."""

    def __init__(self, device_id: int = 0):
        self._h = c_void_p()
        self._batches = weakref.WeakSet()
        self._replay_shape = None      # (P, D, R) of the last replay on this handle (replay_summary sizes its arrays by it)
        rc = lib.tp_create(int(device_id), ctypes.byref(self._h))
        if rc != TP_OK:
            raise TangencyError(rc, lib.tp_last_error(None).decode())
        self.device_id = device_id
        with _live_lock:
            _live_devices.add(self)

    def set_option(self, name: str, value: int):
        """`tp_set_option`: kernel-selection switches of this handle ("wave_kernel", "tiled_wave", "tiled_fuse",
        "wave_preload", "shared_tables", "no_shared_gram", "tiled_arena_gib", "tiled_arena_mib", "hf_share_min_blocks",
        "sweep_chunk_windows": windows per sub-range of `Batch.solve_sweep`, 0 = automatic); the TP_* environment
        variables are read once, when the Device is created.  "shared_tables": 1 = a register-tile batch with shared sums
        builds its block-window tables in one kernel straight from the daily panel, 0 = with the pair of kernels used
        before, -1 (default) = the one kernel at the tile counts where it measured faster; the tables are the same bit
        for bit.  An unknown name or a value an option does not take raises TangencyError."""
        self._check(lib.tp_set_option(self._h, name.encode(), int(value)))
        return self

    def get_option(self, name: str) -> int:
        """`tp_get_option`: the current value of an option, or of the read-only "last_shared_tables" (what built the
        tables of the last register-tile run: 1 the one kernel, 0 the pair, -1 none)."""
        v = c_int()
        self._check(lib.tp_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def _check(self, rc):
        if rc != TP_OK:
            raise TangencyError(rc, lib.tp_last_error(self._h).decode())

    def close(self):
        if self._h:
            for b in list(self._batches):      # a batch must not outlive its handle (tp_destroy would take it down too)
                b.close()
            lib.tp_destroy(self._h)
            self._h = c_void_p()
        with _live_lock:
            _live_devices.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if _finalizing():        # see "lifetime" above: never call into HIP / RCCL from a finaliser at exit
            return
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        name = ctypes.create_string_buffer(256)
        cu, mhz, hbm = c_int(), c_int(), c_int64()
        self._check(lib.tp_device_info(self._h, name, 256, ctypes.byref(cu), ctypes.byref(mhz), ctypes.byref(hbm)))
        return dict(name=name.value.decode(), compute_units=cu.value, clock_mhz=mhz.value, hbm_bytes=hbm.value)

    def synchronize(self):
        self._check(lib.tp_synchronize(self._h))

    def last_timing(self) -> dict:
        v = [c_double() for _ in range(4)]
        self._check(lib.tp_last_timing(self._h, *[ctypes.byref(x) for x in v]))
        return dict(kernel_ms=v[0].value, h2d_ms=v[1].value, d2h_ms=v[2].value, gather_ms=v[3].value)

    def last_launch(self) -> dict:
        v = [c_int() for _ in range(4)]
        self._check(lib.tp_last_launch(self._h, *[ctypes.byref(x) for x in v]))
        return dict(grid=v[0].value, block=v[1].value, lds_bytes=v[2].value, ntile=v[3].value)

    def region_begin(self):
        self._check(lib.tp_region_begin(self._h))

    def region_end(self) -> float:
        ms = c_double()
        self._check(lib.tp_region_end(self._h, ctypes.byref(ms)))
        return ms.value

    def region_steps(self) -> np.ndarray:
        """Kernel milliseconds of every `run` inside the last region_begin / region_end bracket (HIP events per launch)."""
        n = c_int()
        self._check(lib.tp_region_steps(self._h, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        if n.value:
            self._check(lib.tp_region_steps(self._h, _ptr(out, c_double), n.value, ctypes.byref(n)))
        return out

    # ---- RCCL -------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        rc = lib.tp_comm_unique_id(buf)
        if rc != TP_OK:
            raise TangencyError(rc, "ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        buf = ctypes.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        self._check(lib.tp_comm_init(self._h, buf, int(rank), int(world)))
        self.rank, self.world = rank, world

    def comm_destroy(self):
        self._check(lib.tp_comm_destroy(self._h))

    def comm_count(self) -> int:
        """Ranks of the handle's RCCL communicator (ncclCommCount)."""
        n = c_int()
        self._check(lib.tp_comm_count(self._h, ctypes.byref(n)))
        return n.value

    # ---- price front-end ----------------------------------------------------------------------
    def log_returns(self, prices, num, den) -> np.ndarray:
        """out[i] = log(prices[num[i]] / prices[den[i]]) on the device (NaN -> 0), ref:44 / ref:311."""
        P = _arr(prices, np.float64)
        if P.ndim != 2:
            raise ValueError("prices must be 2-D [rows x assets]")
        num, den = _arr(num, np.int32), _arr(den, np.int32)
        if num.ndim != 1 or num.shape != den.shape:
            raise ValueError("num / den: two equally long 1-D index arrays expected")
        out = np.empty((num.size, P.shape[1]), dtype=np.float64)
        self._check(lib.tp_log_returns(self._h, _ptr(P, c_double), P.shape[0], P.shape[1], _ptr(num, c_int32),
                                       _ptr(den, c_int32), num.size, _ptr(out, c_double)))
        return out

    # ---- backtest replay ----------------------------------------------------------------------
    def replay(self, S, rf_daily, reb_day, K, k, scaling, cost, w_off, w_stride, u_off, u_stride, weights, cols, caps,
               download=True):
        """`tp_replay_run` + `tp_replay_download`: daily P&L, weight drift, turnover and weight metrics of P portfolios that
        share trading days and a rebalancing schedule, one wavefront each.  `S` [D x ld] simple returns (the first `K` columns
        are tickers), `rf_daily` [D], `reb_day` [R] trading-day indices (strictly increasing from 0, below D).  Portfolio p
        holds `k[p]` assets; at rebalancing date j its weights are `weights.flat[w_off[p] + j * w_stride[p] + i]`, its tickers
        and their caps `cols.flat[...]` / `caps.flat[u_off[p] + j * u_stride[p] + i]` (cols and caps have one shape).  Every
        check is made before any device call.  Returns (returns [P, D], turnover [P, R], metrics [P, R, 5], status [P],
        bad_day [P]); returns[:, 0] and turnover[:, 0] are NaN; status REPLAY_SUM_CHECK: the weights of that portfolio stopped
        summing to 1 on day bad_day (the host replay raises there).  `download=False`: nothing is returned and nothing is
        copied; the results stay on the device for `replay_summary` (and `_replay_download`)."""
        S, D, ld, K, rf, reb, R, kk, P, sc, co = _replay_schedule(S, rf_daily, reb_day, K, k, scaling, cost)
        wo, wst, uo, ust = (_replay_integer(name, a, np.int64, (P,)) for name, a in
                            (("w_off", w_off), ("w_stride", w_stride), ("u_off", u_off), ("u_stride", u_stride)))
        wts = _replay_real("weights", weights).reshape(-1)
        cl = _replay_integer("cols", cols, np.int32).reshape(-1)
        cp = _replay_real("caps", caps).reshape(-1)
        if cl.size != cp.size:
            raise ValueError(f"cols and caps: one shape expected, got {cl.size} and {cp.size} elements")
        _replay_rows_fit("w", wo, wst, R, kk, wts.size)
        _replay_rows_fit("u", uo, ust, R, kk, cl.size)
        # (the column indices themselves are checked by the library, on the host, while it builds the merge maps)
        nz = lambda a, ct: _ptr(a if a.size else None, ct)   # noqa: E731
        self._check(lib.tp_replay_run(self._h, D, ld, _ptr(S, c_double), _ptr(rf, c_double), R, _ptr(reb, c_int32), K, P,
                                      nz(kk, c_int32), nz(sc, c_double), nz(co, c_double), nz(wo, c_int64), nz(wst, c_int64),
                                      nz(uo, c_int64), nz(ust, c_int64), nz(wts, c_double), wts.size, nz(cl, c_int32),
                                      nz(cp, c_double), cl.size))
        self._replay_shape = (P, D, R)
        return self._replay_download(P, D, R) if download else None

    def replay_summary(self, cost_bp, rf_excess):
        """`tp_replay_summary` + `tp_replay_download_summary` of the last replay on this handle (`replay`, `Batch.replay`, with
        `download=False` or not): the performance statistics of every portfolio's daily returns at every trading cost of
        `cost_bp` [C] (basis points, finite, C <= SUMMARY_MAX_COSTS), with `rf_excess` [D] the daily risk-free rate the excess
        returns subtract (NaN allowed: SUMMARY_NONFINITE).  The costs are applied on the device to the replay's own returns and
        turnover - replay at cost 0.  Returns (stats [P, C, SUMMARY_STATS], status [P, C]); include/tangency_posterior.h
        defines the fields, `portfolio_evaluation.performance_table` turns them into the reference's metrics."""
        if self._replay_shape is None:
            raise ValueError("replay_summary: no replay on this device yet")
        P, D, _R = self._replay_shape
        co = _replay_real("cost_bp", cost_bp)
        rf = _replay_real("rf_excess", rf_excess)
        if co.ndim != 1 or not 1 <= co.size <= SUMMARY_MAX_COSTS:
            raise ValueError(f"cost_bp: 1 to {SUMMARY_MAX_COSTS} costs in a 1-D array expected, got shape {tuple(co.shape)}")
        if not np.isfinite(co).all():
            raise ValueError("cost_bp: finite costs expected")
        if rf.shape != (D,):
            raise ValueError(f"rf_excess: expected shape ({D},), got {tuple(rf.shape)}")
        C = int(co.size)
        self._check(lib.tp_replay_summary(self._h, C, _ptr(co, c_double), _ptr(rf, c_double)))
        stats = np.empty((P, C, SUMMARY_STATS), dtype=np.float64)
        status = np.empty((P, C), dtype=np.int32)
        nz = lambda a, ct: _ptr(a if a.size else None, ct)   # noqa: E731
        self._check(lib.tp_replay_download_summary(self._h, nz(stats, c_double), nz(status, c_int32)))
        return stats, status

    def _replay_download(self, P, D, R):
        """`tp_replay_download`: the results of the last replay on this handle (`replay`, `Batch.replay`)."""
        returns = np.empty((P, D), dtype=np.float64)
        turnover = np.empty((P, R), dtype=np.float64)
        metrics = np.empty((P, R, REPLAY_METRICS), dtype=np.float64)
        status = np.empty(P, dtype=np.int32)
        bad_day = np.empty(P, dtype=np.int32)
        nz = lambda a, ct: _ptr(a if a.size else None, ct)   # noqa: E731
        self._check(lib.tp_replay_download(self._h, nz(returns, c_double), nz(turnover, c_double), nz(metrics, c_double),
                                           nz(status, c_int32), nz(bad_day, c_int32)))
        return returns, turnover, metrics, status, bad_day

    # ---- batches ------------------------------------------------------------------------------
    def batch(self, strategy, k, N, n_r, gamma, W, m=0, flags=0) -> "Batch":
        return Batch(self, strategy, k, N, n_r, gamma, W, m, flags)


class Batch:
    """W windows resident in HBM (`tp_batch_t`)."""

    def __init__(self, dev: Device, strategy, k, N, n_r, gamma, W, m=0, flags=0):
        self.dev = dev
        strat = {"conjugate": STRATEGY_CONJUGATE, "jeffreys": STRATEGY_JEFFREYS}.get(strategy, strategy)
        self.params = tp_params_t(int(k), int(N), int(n_r), int(m), int(strat), int(flags), float(gamma))
        self.W, self.k, self.n_r, self.m = int(W), int(k), int(n_r), int(m)
        self._b = c_void_p()
        dev._check(lib.tp_batch_create(dev._h, ctypes.byref(self.params), self.W, ctypes.byref(self._b)))
        dev._batches.add(self)
        self._keep = None
        self._post = (0, 0)          # window range of keep_posterior

    def close(self):
        if self._b:
            if self.dev._h:                    # a closed Device took its batches with it
                lib.tp_batch_destroy(self._b)
            self._b = c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def upload(self, panel, start=None, hf_panel=None, hf_start=None, w0=None, n0=None, row_idx=None,
               n_rows=None, col_idx=None, rf_adj=None, hf_row_idx=None, hf_count=None, ret_pairs=None,
               hf_ret_pairs=None, asynchronous=False):
        """H2D.  `ret_pairs=(num, den)`: `panel` holds PRICES and the device forms the log-return panel
        R[i] = log(P[num[i]] / P[den[i]]) that start / row_idx address; `hf_ret_pairs` likewise for `hf_panel`."""
        W, k, n_r, m = self.W, self.k, self.n_r, self.m
        panel = _arr(panel, np.float64)
        if panel.ndim != 2:
            raise ValueError("panel must be 2-D [rows x assets]")
        hf_panel = _arr(hf_panel, np.float64)
        if hf_panel is not None and hf_panel.ndim != 2:
            raise ValueError("hf_panel must be 2-D [rows x assets]")
        a = dict(
            panel=panel, hf_panel=hf_panel,
            start=_arr(start, np.int64, (W,), "start"), row_idx=_arr(row_idx, np.int32, (W, n_r), "row_idx"),
            n_rows=_arr(n_rows, np.int32, (W,), "n_rows"), col_idx=_arr(col_idx, np.int32, (W, k), "col_idx"),
            rf_adj=_arr(rf_adj, np.float64, (W, n_r), "rf_adj"),
            hf_start=_arr(hf_start, np.int64, (W,), "hf_start"),
            hf_row_idx=_arr(hf_row_idx, np.int32, (W, m), "hf_row_idx"),
            hf_count=_arr(hf_count, np.int32, (W,), "hf_count"),
            w0=_arr(w0, np.float64, (W, k), "w0"), n0=_arr(n0, np.float64, (W,), "n0"))
        for name, pairs in (("ret", ret_pairs), ("hf_ret", hf_ret_pairs)):
            num = _arr(pairs[0], np.int32) if pairs is not None else None
            den = _arr(pairs[1], np.int32) if pairs is not None else None
            if pairs is not None and (num.ndim != 1 or num.shape != den.shape or num.size < 1):
                raise ValueError(f"{name}_pairs: two equally long 1-D index arrays expected")
            a[name + "_num"], a[name + "_den"] = num, den
        inp = tp_inputs_t(
            _ptr(a["panel"], c_double), panel.shape[0], panel.shape[1],
            hf_panel.shape[1] if hf_panel is not None else 0,
            _ptr(a["start"], c_int64), _ptr(a["row_idx"], c_int32), _ptr(a["n_rows"], c_int32),
            _ptr(a["col_idx"], c_int32), _ptr(a["rf_adj"], c_double),
            _ptr(a["hf_panel"], c_double), hf_panel.shape[0] if hf_panel is not None else 0,
            _ptr(a["hf_start"], c_int64), _ptr(a["hf_row_idx"], c_int32), _ptr(a["hf_count"], c_int32),
            _ptr(a["w0"], c_double), _ptr(a["n0"], c_double),
            _ptr(a["ret_num"], c_int32), _ptr(a["ret_den"], c_int32), a["ret_num"].size if a["ret_num"] is not None else 0,
            _ptr(a["hf_ret_num"], c_int32), _ptr(a["hf_ret_den"], c_int32),
            a["hf_ret_num"].size if a["hf_ret_num"] is not None else 0)
        self._keep = a     # host arrays stay alive for the duration of the upload
        if asynchronous:
            self.dev._check(lib.tp_batch_upload_async(self._b, ctypes.byref(inp)))   # `upload_wait` releases them
        else:
            self.dev._check(lib.tp_batch_upload(self._b, ctypes.byref(inp)))
            self._keep = None
        return self

    def upload_async(self, panel, **kw):
        """`upload` queued on the device's copy stream and not waited for (arrays from `pinned_empty` make the
        copies truly asynchronous).  The next `run` waits for them on the device; `upload_wait` on the host."""
        return self.upload(panel, asynchronous=True, **kw)

    def upload_wait(self):
        self.dev._check(lib.tp_batch_upload_wait(self._b))
        self._keep = None
        return self

    def shared_gram_blocks(self) -> int:
        """Aligned row blocks of the daily panel whose Gram sums this batch's windows share (0: none)."""
        return int(lib.tp_batch_shared_gram_blocks(self._b))

    def shared_intraday_blocks(self) -> int:
        """Large-k path, conjugate: whole intraday blocks (days) per window taken from shared block Grams (0: none)."""
        return int(lib.tp_batch_shared_intraday_blocks(self._b))

    def addressing(self) -> tuple:
        """`tp_batch_addressing` after an upload: (daily, intraday) flag words of `addressing_flags` as the next launch sees
        them; the intraday word is 0 for a batch without an intraday panel."""
        pf, hf = c_int(), c_int()
        self.dev._check(lib.tp_batch_addressing(self._b, ctypes.byref(pf), ctypes.byref(hf)))
        return pf.value, hf.value

    def keep_rhs(self, on=True):
        """Keep the right-hand side every window is solved for in later runs (`download_rhs` reads the last run's)."""
        self.dev._check(lib.tp_batch_keep_rhs(self._b, 1 if on else 0))
        return self

    def keep_posterior(self, begin=0, count=None):
        """Keep the k x k matrix every window of [begin, begin + count) factorises (S1, or J for Jeffreys, shift included)
        in later runs; count None: to the end of the batch, 0: stop.  `download_posterior` reads the last run's."""
        begin = int(begin)
        count = self.W - begin if count is None else int(count)
        self.dev._check(lib.tp_batch_keep_posterior(self._b, begin, count))
        self._post = (begin, count)
        return self

    def download_posterior(self, out=None) -> np.ndarray:
        """[count x k x k] matrices kept by the last run (`keep_posterior` before it).  `out`: a C-contiguous float64
        array of that shape (e.g. `pinned_empty`) to write into."""
        shape = (self._post[1], self.k, self.k)
        if out is not None:
            if out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError(f"out: C-contiguous float64 {shape} expected")
        else:
            out = np.empty(shape, dtype=np.float64)
        buf = out if out.size else np.empty(1, dtype=np.float64)     # (the library reports a missing keep / run)
        self.dev._check(lib.tp_batch_download_posterior(self._b, _ptr(buf, c_double)))
        return out

    def set_rhs(self, rhs):
        """Right-hand side [W x k] in place of the border column (None: default t / c S0 w0 + t).  Jeffreys: the weights
        become (matrix)^-1 rhs / gamma.  Conjugate: rhs replaces c S0 w0 + t in w1 = S1^-1 rhs and the nu rescale of
        ref:572-575 still applies, weights = (n1 + k + 2) w1 / (n1 - w1'S1 w1) / gamma (`solve_sweep` gives S1^-1 rhs / gamma)."""
        r = _arr(rhs, np.float64, (self.W, self.k), "rhs")
        self.dev._check(lib.tp_batch_set_rhs(self._b, _ptr(r, c_double)))
        return self

    def set_shift(self, shift):
        """Per-window (d, e) [W x 2]: the Jeffreys matrix becomes J + d I + e 1 1' (None: no shift)."""
        sh = _arr(shift, np.float64, (self.W, 2), "shift")
        self.dev._check(lib.tp_batch_set_shift(self._b, _ptr(sh, c_double)))
        return self

    def download_rhs(self) -> np.ndarray:
        """[W x k] right-hand sides the windows were solved for in the last run (t = X'1 by default); needs
        `keep_rhs()` before that run."""
        out = np.empty((self.W, self.k), dtype=np.float64)
        self.dev._check(lib.tp_batch_download_rhs(self._b, _ptr(out, c_double)))
        return out

    def run(self):
        self.dev._check(lib.tp_batch_run(self._b))
        return self

    def solve_sweep(self, shift=None, rhs=None, default_rhs=True, out=None, download=True):
        """`tp_batch_solve_sweep` + `tp_batch_download_sweep`: x[w, s, r] = (M_w + d_ws I + e_ws 1 1')^-1 rhs_wr / gamma
        from ONE Gram pass, for `shift` [W x S x 2] = (d, e) (Jeffreys only; None: one unshifted solve) and the
        right-hand sides `rhs` [W x n x k] (a [W x k] array is one column), behind the window's own right-hand side when
        `default_rhs`.  Returns (x [W, S, R, k], status [W, S]).  `out=(x, status)`: write into these arrays (e.g.
        `pinned_empty`).  The batch's results, settings and kept arrays are left alone.  `download=False`: the sweep is queued
        and None returned - the solutions stay on the device for `sweep_finish` (or a later `download_sweep_rhs`)."""
        return self._solve_sweep(lib.tp_batch_solve_sweep, shift, rhs, default_rhs, out, download)

    def solve_sweep_tiled(self, shift=None, rhs=None, default_rhs=True, out=None, download=True):
        """`tp_batch_solve_sweep_tiled` + `tp_batch_download_sweep`: `solve_sweep` for k above `sweep_max_assets()`, every
        (window, shift) pair factorised once by the large-k tiled pipeline with the R right-hand sides riding along as
        columns k .. k+R-1 of the arena (smaller k, or k + R > max_assets() + 1: TP_ERR_UNSUPPORTED).  Same arguments,
        shape checks and return values; `download_sweep_rhs` serves both calls."""
        return self._solve_sweep(lib.tp_batch_solve_sweep_tiled, shift, rhs, default_rhs, out, download)

    def _solve_sweep(self, call, shift, rhs, default_rhs, out, download=True):
        W, k = self.W, self.k
        sh = None
        S = 1
        if shift is not None:
            sh = np.ascontiguousarray(shift, dtype=np.float64)
            if sh.ndim != 3 or sh.shape[0] != W or sh.shape[1] < 1 or sh.shape[2] != 2:
                raise ValueError(f"shift: expected shape ({W}, S, 2) with S >= 1, got {tuple(sh.shape)}")
            S = sh.shape[1]
        r = None
        n_rhs = 0
        if rhs is not None:
            r = np.ascontiguousarray(rhs, dtype=np.float64)
            if r.ndim == 2:
                r = r[:, None, :]
            if r.ndim != 3 or r.shape[0] != W or r.shape[2] != k:
                raise ValueError(f"rhs: expected shape ({W}, n, {k}), got {tuple(r.shape)}")
            r = np.ascontiguousarray(r)
            n_rhs = r.shape[1]
        R = (1 if default_rhs else 0) + n_rhs
        if R < 1 or R > SWEEP_MAX_RHS:
            raise ValueError(f"{R} right-hand sides per window: between 1 and {SWEEP_MAX_RHS} expected")
        if not download:
            if out is not None:
                raise ValueError("out: nothing is downloaded with download=False")
            self.dev._check(call(self._b, S if sh is not None else 0, _ptr(sh, c_double), n_rhs,
                                 _ptr(r if n_rhs else None, c_double), 1 if default_rhs else 0))
            self._sweep_S, self._sweep_R = S, R
            return None
        if out is not None:
            x, status = out
            if x.shape != (W, S, R, k) or x.dtype != np.float64 or not x.flags.c_contiguous:
                raise ValueError(f"out[0]: C-contiguous float64 {(W, S, R, k)} expected")
            if status.shape != (W, S) or status.dtype != np.int32 or not status.flags.c_contiguous:
                raise ValueError(f"out[1]: C-contiguous int32 {(W, S)} expected")
        else:
            x = np.empty((W, S, R, k), dtype=np.float64)
            status = np.empty((W, S), dtype=np.int32)
        self.dev._check(call(self._b, S if sh is not None else 0, _ptr(sh, c_double), n_rhs,
                             _ptr(r if n_rhs else None, c_double), 1 if default_rhs else 0))
        self._sweep_S, self._sweep_R = S, R
        self.dev._check(lib.tp_batch_download_sweep(self._b, _ptr(x if x.size else None, c_double),
                                                    _ptr(status if status.size else None, c_int32)))
        return x, status

    def download_sweep(self):
        """(x [W, S, R, k], status [W, S]) of the last `solve_sweep` / `solve_sweep_tiled`, e.g. one queued with
        `download=False`; the shape is that sweep's."""
        S, R = getattr(self, "_sweep_S", 0), getattr(self, "_sweep_R", 0)
        if S < 1 or R < 1:
            raise ValueError("download_sweep: no solve sweep of this batch yet")
        x = np.empty((self.W, S, R, self.k), dtype=np.float64)
        status = np.empty((self.W, S), dtype=np.int32)
        self.dev._check(lib.tp_batch_download_sweep(self._b, _ptr(x if x.size else None, c_double),
                                                    _ptr(status if status.size else None, c_int32)))
        return x, status

    def sweep_finish(self, mode, n, gamma, kappa=None, xi=None, eta=None):
        """`tp_batch_sweep_finish`: the Greyserman (`FINISH_GREYSERMAN`: `n` [W], `kappa` [W], `xi` and `eta` [W x S]) or
        Jorion (`FINISH_JORION`: `n` [W] = the windows' row counts, S = 1) weights from the solutions the last
        `solve_sweep` / `solve_sweep_tiled` of this batch left on the device - R = 2: `default_rhs=True` and ONE caller
        column, which must be the ones vector; the batch created with gamma = 1, `gamma` is the finish's own.  Nothing comes
        down: `download_sweep_finish` fetches [W x k], `replay(REPLAY_SRC_SWEEP_FINISH, ...)` reads them where they lie.
        Shapes are checked here; the library refuses the rest (TangencyError, code ERR_INVALID) before it queues anything."""
        W = self.W
        mode = int(mode)
        nn = np.ascontiguousarray(n, dtype=np.float64)
        if nn.shape != (W,):
            raise ValueError(f"n: expected shape ({W},), got {tuple(nn.shape)}")
        ka = hy = None
        if mode == FINISH_GREYSERMAN:
            if kappa is None or xi is None or eta is None:
                raise ValueError("sweep_finish(FINISH_GREYSERMAN): kappa, xi and eta are needed")
            ka = np.ascontiguousarray(kappa, dtype=np.float64)
            x_, e_ = np.asarray(xi, dtype=np.float64), np.asarray(eta, dtype=np.float64)
            if ka.shape != (W,):
                raise ValueError(f"kappa: expected shape ({W},), got {tuple(ka.shape)}")
            if x_.ndim != 2 or x_.shape[0] != W or e_.shape != x_.shape:
                raise ValueError(f"xi, eta: expected one shape ({W}, S), got {tuple(x_.shape)} and {tuple(e_.shape)}")
            if x_.shape[1] != getattr(self, "_sweep_S", x_.shape[1]):
                raise ValueError(f"xi, eta: {x_.shape[1]} draws per window, the last sweep had {self._sweep_S} shifts")
            hy = np.ascontiguousarray(np.stack([x_, e_], axis=2))
        self.dev._check(lib.tp_batch_sweep_finish(self._b, mode, float(gamma), _ptr(nn if nn.size else None, c_double),
                                                  _ptr(ka if ka is not None and ka.size else None, c_double),
                                                  _ptr(hy if hy is not None and hy.size else None, c_double)))
        self._finish_S = getattr(self, "_sweep_S", 1)
        return self

    def download_sweep_finish(self, want_aux=False):
        """(weights [W x k], status [W], aux [W x S x 4] or None) of the last `sweep_finish`: aux[w, s] = (1'u_one, 1'u_t,
        t'u_t, det K) - Jorion: q in the fourth slot."""
        weights = np.empty((self.W, self.k), dtype=np.float64)
        status = np.empty(self.W, dtype=np.int32)
        aux = np.empty((self.W, getattr(self, "_finish_S", 1), 4), dtype=np.float64) if want_aux else None
        self.dev._check(lib.tp_batch_download_sweep_finish(self._b, _ptr(weights if weights.size else None, c_double),
                                                           _ptr(status if status.size else None, c_int32),
                                                           _ptr(aux if aux is not None and aux.size else None, c_double)))
        return weights, status, aux

    def spectral_greyserman(self, n, gamma, kappa, xi, eta, keep_vectors=False):
        """`tp_batch_spectral_greyserman`: the Greyserman weights of the draws `xi`, `eta` [W x S] (`n`, `kappa` [W]) from ONE
        eigendecomposition per window - the ridge shifts eta / 2 share the eigenvectors of the window's matrix - instead of S
        factorisations; no solve sweep before it, no W x S x 2 x k solutions.  A Jeffreys batch created with gamma = 1,
        k <= `sweep_max_assets()`; `gamma` is the call's own.  `keep_vectors`: the eigenvectors of every window are kept for
        `download_spectral(want_vectors=True)`.  Nothing comes down: `download_spectral` fetches the results,
        `replay(REPLAY_SRC_SPECTRAL, ...)` reads the weights where they lie.  Shapes are checked here; the library refuses the
        rest (TangencyError) before it queues anything."""
        W = self.W
        nn = np.ascontiguousarray(n, dtype=np.float64)
        ka = np.ascontiguousarray(kappa, dtype=np.float64)
        x_, e_ = np.asarray(xi, dtype=np.float64), np.asarray(eta, dtype=np.float64)
        if nn.shape != (W,):
            raise ValueError(f"n: expected shape ({W},), got {tuple(nn.shape)}")
        if ka.shape != (W,):
            raise ValueError(f"kappa: expected shape ({W},), got {tuple(ka.shape)}")
        if x_.ndim != 2 or x_.shape[0] != W or e_.shape != x_.shape:
            raise ValueError(f"xi, eta: expected one shape ({W}, S), got {tuple(x_.shape)} and {tuple(e_.shape)}")
        S = x_.shape[1]
        hy = np.ascontiguousarray(np.stack([x_, e_], axis=2))
        self.dev._check(lib.tp_batch_spectral_greyserman(self._b, S, float(gamma), _ptr(nn if nn.size else None, c_double),
                                                         _ptr(ka if ka.size else None, c_double),
                                                         _ptr(hy if hy.size else None, c_double), 1 if keep_vectors else 0))
        self._spectral_S = S
        return self

    def download_spectral(self, want_aux=False, want_spectrum=False, want_vectors=False):
        """(weights [W x k], status [W], aux [W x S x 4] or None) of the last `spectral_greyserman`: aux[w, s] = (s1, s2, s3,
        det K).  `want_spectrum`: (lambda [W x k] - not sorted -, sweeps [W]) are appended; `want_vectors` (the call needs
        `keep_vectors=True`): V [W x k x k] with V[w, :, j] the eigenvector of lambda[w, j]."""
        W, k = self.W, self.k
        weights = np.empty((W, k), dtype=np.float64)
        status = np.empty(W, dtype=np.int32)
        aux = np.empty((W, getattr(self, "_spectral_S", 1), 4), dtype=np.float64) if want_aux else None
        lam = np.empty((W, k), dtype=np.float64) if want_spectrum else None
        sweeps = np.empty(W, dtype=np.int32) if want_spectrum else None
        V = np.empty((W, k, k), dtype=np.float64) if want_vectors else None
        opt = lambda a, t: _ptr(a if a is not None and a.size else None, t)   # noqa: E731
        self.dev._check(lib.tp_batch_download_spectral(self._b, opt(weights, c_double), opt(status, c_int32), opt(aux, c_double),
                                                       opt(lam, c_double), opt(sweeps, c_int32), opt(V, c_double)))
        out = (weights, status, aux)
        if want_spectrum:
            out += (lam, sweeps)
        if want_vectors:
            out += (V.transpose(0, 2, 1),)                   # (the library's layout is column-major per window)
        return out

    def download_sweep_rhs(self) -> np.ndarray:
        """[W x k] default right-hand sides (t = X'1, or c S0 w0 + t) the Gram pass of the last `solve_sweep` /
        `solve_sweep_tiled` formed."""
        out = np.empty((self.W, self.k), dtype=np.float64)
        self.dev._check(lib.tp_batch_download_sweep_rhs(self._b, _ptr(out if out.size else None, c_double)))
        return out

    def prior_sweep(self, n0, w0, want_aux=True, want_weights=True):
        """`tp_batch_prior_sweep` + `tp_batch_download_prior_sweep`: the conjugate weights of every window for P priors
        `n0` [W x P] (> 0), `w0` [W x P x k] from ONE pair of Grams per window.  Returns (weights [W, P, k], status [W, P],
        aux [W, P, 8] or None).  The batch's own w0 / n0, results, settings and kept arrays are left alone.
        `want_weights=False` (every sweep method): the weights stay on the device - for `replay` - and None is returned in
        their place."""
        return self._prior_sweep(lib.tp_batch_prior_sweep, n0, w0, want_aux, want_weights)

    def prior_sweep_tiled(self, n0, w0, want_aux=True, want_weights=True):
        """`tp_batch_prior_sweep_tiled` + `tp_batch_download_prior_sweep`: `prior_sweep` for k above `sweep_max_assets()`,
        factorised by the large-k tiled pipeline (smaller k: TP_ERR_UNSUPPORTED).  The intraday scatter is centred through
        the raw moments: meant for returns, not for panels with a large common offset."""
        return self._prior_sweep(lib.tp_batch_prior_sweep_tiled, n0, w0, want_aux, want_weights)

    def _prior_sweep(self, call, n0, w0, want_aux, want_weights=True):
        W, k = self.W, self.k
        for name, a in (("n0", n0), ("w0", w0)):
            if a is None:
                raise ValueError(f"{name}: an array is expected")
            if np.asarray(a).dtype.kind not in "fiu":
                raise ValueError(f"{name}: a real floating-point array is expected, got dtype {np.asarray(a).dtype}")
        n0 = np.ascontiguousarray(n0, dtype=np.float64)
        w0 = np.ascontiguousarray(w0, dtype=np.float64)
        if n0.ndim != 2 or n0.shape[0] != W or n0.shape[1] < 1:
            raise ValueError(f"n0: expected shape ({W}, P) with P >= 1, got {tuple(n0.shape)}")
        P = n0.shape[1]
        if w0.shape != (W, P, k):
            raise ValueError(f"w0: expected shape ({W}, {P}, {k}), got {tuple(w0.shape)}")
        weights = np.empty((W, P, k), dtype=np.float64) if want_weights else None
        status = np.empty((W, P), dtype=np.int32)
        aux = np.empty((W, P, AUX_STRIDE), dtype=np.float64) if want_aux else None
        # (W = 0: the library still wants non-NULL prior arrays)
        n0p = n0 if n0.size else np.ones(1)
        w0p = w0 if w0.size else np.zeros(1)
        self.dev._check(call(self._b, P, _ptr(n0p, c_double), _ptr(w0p, c_double)))
        self.dev._check(lib.tp_batch_download_prior_sweep(self._b, _ptr(weights if weights is not None and weights.size else None, c_double),
                                                          _ptr(status if status.size else None, c_int32),
                                                          _ptr(aux if aux is not None and aux.size else None, c_double)))
        return weights, status, aux

    def size_sweep(self, sizes, n0=None, w0=None, want_aux=True, want_weights=True):
        """`tp_batch_size_sweep` + `tp_batch_download_size_sweep`: S nested universes per window - the first `sizes[s]`
        columns, strictly increasing within [1, k], at most SWEEP_MAX_RHS of them - from ONE factorisation per (window,
        prior).  Conjugate batch: `n0` [W x P] (> 0), `w0` [W x P x S x k] (only the first sizes[s] entries of a vector are
        read).  Jeffreys batch: no priors, P = 1.  Returns (weights [W, P, S, k] - zero beyond sizes[s] -, status [W, P, S],
        aux [W, P, S, 8] or None).  The batch's results, settings and kept arrays are left alone."""
        return self._size_sweep(lib.tp_batch_size_sweep, sizes, n0, w0, want_aux, want_weights)

    def size_sweep_tiled(self, sizes, n0=None, w0=None, want_aux=True, want_weights=True):
        """`tp_batch_size_sweep_tiled` + `tp_batch_download_size_sweep`: `size_sweep` for k above `sweep_max_assets()`, every
        (window, prior) factorised once at k by the large-k tiled pipeline with the S right-hand sides riding along as
        columns k .. k+S-1 of the arena (smaller k, or k + S > max_assets() + 1: TP_ERR_UNSUPPORTED).  Same arguments, shape
        checks and return values; single sizes may lie below `sweep_max_assets()`.  A non-finite column j also spoils the
        sizes in (64 floor(j/64), j], which come back flagged; the intraday scatter is centred through the raw moments."""
        return self._size_sweep(lib.tp_batch_size_sweep_tiled, sizes, n0, w0, want_aux, want_weights)

    def _size_sweep(self, call, sizes, n0, w0, want_aux, want_weights=True):
        W, k = self.W, self.k
        if sizes is None or np.asarray(sizes).dtype.kind not in "iu":
            raise ValueError("sizes: a sequence of integers is expected")
        sz = np.ascontiguousarray(sizes, dtype=np.int32)
        if sz.ndim != 1 or not 1 <= sz.size <= SWEEP_MAX_RHS:
            raise ValueError(f"sizes: between 1 and {SWEEP_MAX_RHS} sizes expected, got shape {tuple(sz.shape)}")
        if sz[0] < 1 or sz[-1] > k or (np.diff(sz) <= 0).any():
            raise ValueError(f"sizes: strictly increasing within [1, {k}] expected, got {sz.tolist()}")
        S = int(sz.size)
        if (n0 is None) != (w0 is None):
            raise ValueError("n0 and w0: both (conjugate batch) or neither (Jeffreys batch) expected")
        P = 1
        if n0 is not None:
            for name, a in (("n0", n0), ("w0", w0)):
                if np.asarray(a).dtype.kind not in "fiu":
                    raise ValueError(f"{name}: a real floating-point array is expected, got dtype {np.asarray(a).dtype}")
            n0 = np.ascontiguousarray(n0, dtype=np.float64)
            w0 = np.ascontiguousarray(w0, dtype=np.float64)
            if n0.ndim != 2 or n0.shape[0] != W or n0.shape[1] < 1:
                raise ValueError(f"n0: expected shape ({W}, P) with P >= 1, got {tuple(n0.shape)}")
            P = n0.shape[1]
            if w0.shape != (W, P, S, k):
                raise ValueError(f"w0: expected shape ({W}, {P}, {S}, {k}), got {tuple(w0.shape)}")
        weights = np.empty((W, P, S, k), dtype=np.float64) if want_weights else None
        status = np.empty((W, P, S), dtype=np.int32)
        aux = np.empty((W, P, S, AUX_STRIDE), dtype=np.float64) if want_aux else None
        if n0 is None:
            self.dev._check(call(self._b, S, _ptr(sz, c_int32), 0, None, None))
        else:
            # (W = 0: the library still wants non-NULL prior arrays)
            n0p = n0 if n0.size else np.ones(1)
            w0p = w0 if w0.size else np.zeros(1)
            self.dev._check(call(self._b, S, _ptr(sz, c_int32), P, _ptr(n0p, c_double), _ptr(w0p, c_double)))
        self.dev._check(lib.tp_batch_download_size_sweep(self._b, _ptr(weights if weights is not None and weights.size else None, c_double),
                                                         _ptr(status if status.size else None, c_int32),
                                                         _ptr(aux if aux is not None and aux.size else None, c_double)))
        return weights, status, aux

    def window_sweep(self, N, rows, n0=None, w0=None, delta=None, want_aux=True, want_weights=True):
        return self._window_sweep(lib.tp_batch_window_sweep, N, rows, n0, w0, delta, want_aux, want_weights)

    def window_sweep_tiled(self, N, rows, n0=None, w0=None, delta=None, want_aux=True, want_weights=True):
        """`tp_batch_window_sweep_tiled` + `tp_batch_download_window_sweep`: `window_sweep` for k > `sweep_max_assets()`, on the
        large-k tiled pipeline - the same arguments, checks (before any device call) and results; statuses as `run` gives
        them on the large-k path."""
        return self._window_sweep(lib.tp_batch_window_sweep_tiled, N, rows, n0, w0, delta, want_aux, want_weights)

    def _window_sweep(self, call, N, rows, n0, w0, delta, want_aux, want_weights=True):
        """`tp_batch_window_sweep` + `tp_batch_download_window_sweep`: L nested window lengths per window - length l uses the
        last `rows[w, l]` daily rows of the window as uploaded - from ONE pass over the rows.  `N` [L]: strictly increasing,
        replaces the batch's N per length; `rows` [W x L]: non-decreasing in l within [1, n_w]; `delta` [W x L x n_r] or None:
        subtracted from every column of row r for length l (the length's own risk-free adjustment minus the batch's).
        Conjugate batch: `n0` [W x P x L] (> 0), `w0` [W x P x k].  Jeffreys batch: no priors, P = 1.  Returns
        (weights [W, P, L, k], status [W, P, L], aux [W, P, L, 8] or None).  The batch's results, settings and kept arrays
        and the other sweeps' results are left alone."""
        W, k = self.W, self.k
        if N is None or np.asarray(N).dtype.kind not in "iu":
            raise ValueError("N: a sequence of integers is expected")
        Nl = np.ascontiguousarray(N, dtype=np.int32)
        if Nl.ndim != 1 or not 1 <= Nl.size <= SWEEP_MAX_RHS:
            raise ValueError(f"N: between 1 and {SWEEP_MAX_RHS} lengths expected, got shape {tuple(Nl.shape)}")
        L = int(Nl.size)
        if rows is None or np.asarray(rows).dtype.kind not in "iu":
            raise ValueError("rows: an integer array is expected")
        rw = np.ascontiguousarray(rows, dtype=np.int32)
        if rw.shape != (W, L):
            raise ValueError(f"rows: expected shape ({W}, {L}), got {tuple(rw.shape)}")
        if delta is not None:
            if np.asarray(delta).dtype.kind not in "fiu":
                raise ValueError(f"delta: a real floating-point array is expected, got dtype {np.asarray(delta).dtype}")
            delta = np.ascontiguousarray(delta, dtype=np.float64)
            if delta.shape != (W, L, self.n_r):
                raise ValueError(f"delta: expected shape ({W}, {L}, {self.n_r}), got {tuple(delta.shape)}")
        if (n0 is None) != (w0 is None):
            raise ValueError("n0 and w0: both (conjugate batch) or neither (Jeffreys batch) expected")
        P = 1
        if n0 is not None:
            for name, a in (("n0", n0), ("w0", w0)):
                if np.asarray(a).dtype.kind not in "fiu":
                    raise ValueError(f"{name}: a real floating-point array is expected, got dtype {np.asarray(a).dtype}")
            n0 = np.ascontiguousarray(n0, dtype=np.float64)
            w0 = np.ascontiguousarray(w0, dtype=np.float64)
            if n0.ndim != 3 or n0.shape[0] != W or n0.shape[1] < 1 or n0.shape[2] != L:
                raise ValueError(f"n0: expected shape ({W}, P, {L}) with P >= 1, got {tuple(n0.shape)}")
            P = n0.shape[1]
            if w0.shape != (W, P, k):
                raise ValueError(f"w0: expected shape ({W}, {P}, {k}), got {tuple(w0.shape)}")
        weights = np.empty((W, P, L, k), dtype=np.float64) if want_weights else None
        status = np.empty((W, P, L), dtype=np.int32)
        aux = np.empty((W, P, L, AUX_STRIDE), dtype=np.float64) if want_aux else None
        # (W = 0: the library still wants non-NULL arrays)
        rwp = rw if rw.size else np.ones(1, dtype=np.int32)
        dp = None if delta is None or not delta.size else delta
        if n0 is None:
            self.dev._check(call(self._b, L, _ptr(Nl, c_int32), _ptr(rwp, c_int32), _ptr(dp, c_double), 0, None, None))
        else:
            n0p = n0 if n0.size else np.ones(1)
            w0p = w0 if w0.size else np.zeros(1)
            self.dev._check(call(self._b, L, _ptr(Nl, c_int32), _ptr(rwp, c_int32), _ptr(dp, c_double), P, _ptr(n0p, c_double),
                                 _ptr(w0p, c_double)))
        self.dev._check(lib.tp_batch_download_window_sweep(self._b, _ptr(weights if weights is not None and weights.size else None, c_double),
                                                           _ptr(status if status.size else None, c_int32),
                                                           _ptr(aux if aux is not None and aux.size else None, c_double)))
        return weights, status, aux

    def grid_sweep(self, sizes, N, rows, n0=None, w0=None, delta=None, want_aux=True, want_weights=True):
        return self._grid_sweep(lib.tp_batch_grid_sweep, sizes, N, rows, n0, w0, delta, want_aux, want_weights)

    def grid_sweep_tiled(self, sizes, N, rows, n0=None, w0=None, delta=None, want_aux=True, want_weights=True):
        """`tp_batch_grid_sweep_tiled` + `tp_batch_download_grid_sweep`: `grid_sweep` for k > `sweep_max_assets()`, on the
        large-k tiled pipeline - the same arguments, checks (before any device call) and results; single sizes may lie below
        that bound.  k + len(sizes) <= `max_assets()` + 1."""
        return self._grid_sweep(lib.tp_batch_grid_sweep_tiled, sizes, N, rows, n0, w0, delta, want_aux, want_weights)

    def _grid_sweep(self, call, sizes, N, rows, n0, w0, delta, want_aux, want_weights=True):
        """`tp_batch_grid_sweep` + `tp_batch_download_grid_sweep`: S nested universes x L nested window lengths per window -
        entry (l, s) uses the first `sizes[s]` columns and the last `rows[w, l]` daily rows of the window as uploaded - from ONE
        pass over the rows and ONE factorisation per (window, prior, length).  `sizes` as in `size_sweep`; `N`, `rows` and
        `delta` as in `window_sweep`.  Conjugate batch: `n0` [W x P x L] (> 0), `w0` [W x P x S x k] (only the first sizes[s]
        entries of a vector are read).  Jeffreys batch: no priors, P = 1.  Returns (weights [W, P, L, S, k] - zero beyond
        sizes[s] -, status [W, P, L, S], aux [W, P, L, S, 8] or None; `want_weights=False`: None for the weights, which stay
        on the device for `replay`).  The batch's results, settings and kept arrays and the other sweeps' results are left
        alone."""
        W, k = self.W, self.k
        if sizes is None or np.asarray(sizes).dtype.kind not in "iu":
            raise ValueError("sizes: a sequence of integers is expected")
        sz = np.ascontiguousarray(sizes, dtype=np.int32)
        if sz.ndim != 1 or not 1 <= sz.size <= SWEEP_MAX_RHS:
            raise ValueError(f"sizes: between 1 and {SWEEP_MAX_RHS} sizes expected, got shape {tuple(sz.shape)}")
        if sz[0] < 1 or sz[-1] > k or (np.diff(sz) <= 0).any():
            raise ValueError(f"sizes: strictly increasing within [1, {k}] expected, got {sz.tolist()}")
        S = int(sz.size)
        if N is None or np.asarray(N).dtype.kind not in "iu":
            raise ValueError("N: a sequence of integers is expected")
        Nl = np.ascontiguousarray(N, dtype=np.int32)
        if Nl.ndim != 1 or not 1 <= Nl.size <= SWEEP_MAX_RHS:
            raise ValueError(f"N: between 1 and {SWEEP_MAX_RHS} lengths expected, got shape {tuple(Nl.shape)}")
        L = int(Nl.size)
        if rows is None or np.asarray(rows).dtype.kind not in "iu":
            raise ValueError("rows: an integer array is expected")
        rw = np.ascontiguousarray(rows, dtype=np.int32)
        if rw.shape != (W, L):
            raise ValueError(f"rows: expected shape ({W}, {L}), got {tuple(rw.shape)}")
        if delta is not None:
            if np.asarray(delta).dtype.kind not in "fiu":
                raise ValueError(f"delta: a real floating-point array is expected, got dtype {np.asarray(delta).dtype}")
            delta = np.ascontiguousarray(delta, dtype=np.float64)
            if delta.shape != (W, L, self.n_r):
                raise ValueError(f"delta: expected shape ({W}, {L}, {self.n_r}), got {tuple(delta.shape)}")
        if (n0 is None) != (w0 is None):
            raise ValueError("n0 and w0: both (conjugate batch) or neither (Jeffreys batch) expected")
        P = 1
        if n0 is not None:
            for name, a in (("n0", n0), ("w0", w0)):
                if np.asarray(a).dtype.kind not in "fiu":
                    raise ValueError(f"{name}: a real floating-point array is expected, got dtype {np.asarray(a).dtype}")
            n0 = np.ascontiguousarray(n0, dtype=np.float64)
            w0 = np.ascontiguousarray(w0, dtype=np.float64)
            if n0.ndim != 3 or n0.shape[0] != W or n0.shape[1] < 1 or n0.shape[2] != L:
                raise ValueError(f"n0: expected shape ({W}, P, {L}) with P >= 1, got {tuple(n0.shape)}")
            P = n0.shape[1]
            if w0.shape != (W, P, S, k):
                raise ValueError(f"w0: expected shape ({W}, {P}, {S}, {k}), got {tuple(w0.shape)}")
        weights = np.empty((W, P, L, S, k), dtype=np.float64) if want_weights else None
        status = np.empty((W, P, L, S), dtype=np.int32)
        aux = np.empty((W, P, L, S, AUX_STRIDE), dtype=np.float64) if want_aux else None
        # (W = 0: the library still wants non-NULL arrays)
        rwp = rw if rw.size else np.ones(1, dtype=np.int32)
        dp = None if delta is None or not delta.size else delta
        if n0 is None:
            self.dev._check(call(self._b, S, _ptr(sz, c_int32), L, _ptr(Nl, c_int32), _ptr(rwp, c_int32), _ptr(dp, c_double), 0,
                                 None, None))
        else:
            n0p = n0 if n0.size else np.ones(1)
            w0p = w0 if w0.size else np.zeros(1)
            self.dev._check(call(self._b, S, _ptr(sz, c_int32), L, _ptr(Nl, c_int32), _ptr(rwp, c_int32), _ptr(dp, c_double), P,
                                 _ptr(n0p, c_double), _ptr(w0p, c_double)))
        self.dev._check(lib.tp_batch_download_grid_sweep(self._b, _ptr(weights if weights is not None and weights.size else None, c_double),
                                                         _ptr(status if status.size else None, c_int32),
                                                         _ptr(aux if aux is not None and aux.size else None, c_double)))
        return weights, status, aux

    def replay(self, source, S, rf_daily, reb_day, K, k, scaling, cost, w_off, w_stride, s_off, s_stride, u_off, u_stride,
               cols, caps, w_scale=None, patches=None, download=True):
        """`tp_replay_run_batch` + `tp_replay_download`: `Device.replay` with the weights read where this batch's last run or
        sweep of kind `source` (REPLAY_SRC_*) left them on the device - nothing but the small inputs goes up, nothing but the
        results comes down.  At rebalancing date j portfolio p holds `w_scale[p] * src[w_off[p] + j * w_stride[p] + i]`
        (`w_scale` [P] or None: ones; one rounding, 1.0 leaves the bits alone) and the row's status is
        `srcstatus[s_off[p] + j * s_stride[p]]`, both in elements of the source's results as its download returns them
        (the sweeps' methods take `want_weights=False`).  `patches` = (port [n], date [n], rows [n x patch_ld]) or None: date
        `date[q]` of portfolio `port[q]` holds `rows[q, :k]` instead, unscaled and whatever the source's status; sorted by
        (port, date), strictly.  The other arguments and the returns are `Device.replay`'s; status REPLAY_BAD_WEIGHTS: a row
        was read whose source status was not STATUS_OK, at rebalancing day bad_day (NaN from there on).  Shapes and types are
        checked here, before any device call; the library checks the source, the offsets against the source's counts and the
        patches' order before it uploads or launches anything (TangencyError, code ERR_INVALID).  `download=False`: as
        `Device.replay`."""
        source = int(source)
        S, D, ld, K, rf, reb, R, kk, P, sc, co = _replay_schedule(S, rf_daily, reb_day, K, k, scaling, cost)
        wo, wst, so, sst, uo, ust = (_replay_integer(name, a, np.int64, (P,)) for name, a in
                                     (("w_off", w_off), ("w_stride", w_stride), ("s_off", s_off), ("s_stride", s_stride),
                                      ("u_off", u_off), ("u_stride", u_stride)))
        cl = _replay_integer("cols", cols, np.int32).reshape(-1)
        cp = _replay_real("caps", caps).reshape(-1)
        if cl.size != cp.size:
            raise ValueError(f"cols and caps: one shape expected, got {cl.size} and {cp.size} elements")
        _replay_rows_fit("u", uo, ust, R, kk, cl.size)
        ws = None
        if w_scale is not None:
            ws = _replay_real("w_scale", w_scale)
            if ws.shape != (P,):
                raise ValueError(f"w_scale: expected shape ({P},), got {tuple(ws.shape)}")
        n_patch, pp, pd_, pr, patch_ld = 0, None, None, None, 0
        if patches is not None:
            if len(patches) != 3:
                raise ValueError("patches: (port, date, rows) expected")
            pp = _replay_integer("patches[0]", patches[0], np.int64)
            pd_ = _replay_integer("patches[1]", patches[1], np.int32)
            pr = _replay_real("patches[2]", patches[2], 2)
            n_patch = int(pp.size)
            if pp.ndim != 1 or pd_.shape != (n_patch,) or pr.shape[0] != n_patch:
                raise ValueError(f"patches: port [n], date [n] and rows [n x ld] expected, got {tuple(pp.shape)}, "
                                 f"{tuple(pd_.shape)}, {tuple(pr.shape)}")
            patch_ld = int(pr.shape[1])
        nz = lambda a, ct: _ptr(a if a is not None and a.size else None, ct)   # noqa: E731
        dev = self.dev
        dev._check(lib.tp_replay_run_batch(self._b, source, D, ld, _ptr(S, c_double), _ptr(rf, c_double), R, _ptr(reb, c_int32),
                                           K, P, nz(kk, c_int32), nz(sc, c_double), nz(co, c_double), nz(ws, c_double),
                                           nz(wo, c_int64), nz(wst, c_int64), nz(so, c_int64), nz(sst, c_int64),
                                           nz(uo, c_int64), nz(ust, c_int64), nz(cl, c_int32), nz(cp, c_double), cl.size,
                                           n_patch, nz(pp, c_int64), nz(pd_, c_int32), nz(pr, c_double), patch_ld))
        dev._replay_shape = (P, D, R)
        return dev._replay_download(P, D, R) if download else None

    def download(self, want_aux=True, out=None):
        """(weights, status, aux).  `out=(weights, status[, aux])`: write into these arrays (e.g. `pinned_empty`)."""
        if out is not None:
            weights, status = out[0], out[1]
            aux = out[2] if len(out) > 2 else None
            if weights.shape != (self.W, self.k) or weights.dtype != np.float64 or not weights.flags.c_contiguous:
                raise ValueError("out[0]: C-contiguous float64 [W x k] expected")
            if status.shape != (self.W,) or status.dtype != np.int32:
                raise ValueError("out[1]: int32 [W] expected")
            if aux is not None and (aux.shape != (self.W, AUX_STRIDE) or aux.dtype != np.float64):
                raise ValueError("out[2]: float64 [W x 8] expected")
            self.dev._check(lib.tp_batch_download(self._b, _ptr(weights, c_double), _ptr(status, c_int32),
                                                  _ptr(aux, c_double)))
            return weights, status, aux
        weights = np.empty((self.W, self.k), dtype=np.float64)
        status = np.empty(self.W, dtype=np.int32)
        aux = np.empty((self.W, AUX_STRIDE), dtype=np.float64) if want_aux else None
        self.dev._check(lib.tp_batch_download(self._b, _ptr(weights, c_double), _ptr(status, c_int32),
                                              _ptr(aux, c_double)))
        return weights, status, aux

    def download_S1(self, w: int) -> np.ndarray:
        S1 = np.empty((self.k, self.k), dtype=np.float64)
        self.dev._check(lib.tp_batch_download_S1(self._b, int(w), _ptr(S1, c_double)))
        return S1

    def download_matrix(self, w: int, what):
        """(M [k x k], rhs [k]) of window w: what = 'prior' (S0, c S0 w0), 'gram' (T, t) or
        'posterior' (S1 or J, right-hand side)."""
        code = {"prior": 1, "gram": 2, "posterior": 3}.get(what, what)
        M = np.empty((self.k, self.k), dtype=np.float64)
        rhs = np.empty(self.k, dtype=np.float64)
        self.dev._check(lib.tp_batch_download_matrix(self._b, int(w), int(code), _ptr(M, c_double), _ptr(rhs, c_double)))
        return M, rhs

    def debug_stamps(self) -> np.ndarray:
        """[W x 8] shader-clock stamps at the kernel's phase boundaries (TP_STAMP builds only)."""
        st = np.zeros((self.W, 40), dtype=np.int64)
        self.dev._check(lib.tp_batch_debug_stamps(self._b, _ptr(st, c_int64)))
        return st

    def gather(self, root=0, to_host=True):
        """One RCCL gather of every rank's [W x k] weights (and statuses) to `root`.  With
        `to_host=False` the result stays in root's HBM (`download_gathered` fetches it later)."""
        world, rank = self.dev.world, self.dev.rank
        self._gather_root = root
        if rank == root and to_host:
            wall = np.empty((world, self.W, self.k), dtype=np.float64)
            sall = np.empty((world, self.W), dtype=np.int32)
            self.dev._check(lib.tp_batch_gather(self._b, root, _ptr(wall, c_double), _ptr(sall, c_int32)))
            return wall, sall
        self.dev._check(lib.tp_batch_gather(self._b, root, None, None))
        return None, None

    def gather_async(self, root=0):
        """The same gather on the handle's second stream, not waited for: it overlaps the next `run`.
        `Device.synchronize()` or `download_gathered()` wait for it."""
        self._gather_root = root
        self.dev._check(lib.tp_batch_gather_async(self._b, root))
        return self

    def download_gathered(self):
        world = self.dev.world
        wall = np.empty((world, self.W, self.k), dtype=np.float64)
        sall = np.empty((world, self.W), dtype=np.int32)
        self.dev._check(lib.tp_batch_download_gathered(self._b, _ptr(wall, c_double), _ptr(sall, c_int32)))
        return wall, sall


class DeviceGroup:
    """Every visible GPU of THIS process under one RCCL communicator (`tp_comm_init_all`): the single-process
    multi-device mode behind `backtest_portfolio` (the reference's main.py is one process, src/main.py:26).
    Windows shard contiguously over the devices (`shard.run_sharded`); one grouped gather brings the weights to
    device 0."""

    def __init__(self, device_ids=None):
        ids = list(range(device_count())) if device_ids is None else list(device_ids)
        if not ids:
            raise TangencyError(TP_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback")
        self.devices = [Device(i) for i in ids]
        self.world = len(self.devices)
        if self.world > 1:
            arr = (c_void_p * self.world)(*[d._h for d in self.devices])
            rc = lib.tp_comm_init_all(arr, self.world)
            if rc != TP_OK:
                raise TangencyError(rc, lib.tp_last_error(self.devices[0]._h).decode())
            for r, d in enumerate(self.devices):
                d.rank, d.world = r, self.world

    def gather(self, batches, root=0):
        """One grouped RCCL gather of the equally sized batches (batches[i] on devices[i]) to `root`: returns
        (weights [world x W x k], status [world x W]) on the host."""
        n = len(batches)
        if n != self.world:
            raise ValueError("one batch per device expected")
        if n == 1:
            w, s, _ = batches[0].download(want_aux=False)
            return w[None], s[None]
        W, k = batches[0].W, batches[0].k
        wall = np.empty((n, W, k), dtype=np.float64)
        sall = np.empty((n, W), dtype=np.int32)
        arr = (c_void_p * n)(*[b._b for b in batches])
        rc = lib.tp_group_gather(arr, n, int(root), _ptr(wall, c_double), _ptr(sall, c_int32))
        if rc != TP_OK:
            raise TangencyError(rc, lib.tp_last_error(self.devices[root]._h).decode())
        return wall, sall

    def close(self):
        for d in self.devices:
            d.close()
        self.devices = []


_default_device = None
_default_group = None


def default_group() -> DeviceGroup:
    """All visible GPUs of this process (created on first use; `TP_DEVICES=0,1,..` restricts them)."""
    global _default_group
    if _default_group is None:
        ids = os.environ.get("TP_DEVICES")
        _default_group = DeviceGroup([int(x) for x in ids.split(",")] if ids else None)
    return _default_group


def default_device() -> Device:
    global _default_device
    if _default_device is None:
        _default_device = Device(int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("TP_DEVICE") is None
                                 else int(os.environ["TP_DEVICE"]))
    return _default_device


def posterior_batch(strategy, k, N, gamma, panel, start=None, n_r=None, hf_panel=None, hf_start=None, m=0,
                    w0=None, n0=None, row_idx=None, n_rows=None, col_idx=None, rf_adj=None,
                    hf_row_idx=None, hf_count=None, device: Device | None = None, want_aux=True, rhs=None, flags=0,
                    shift=None, ret_pairs=None, hf_ret_pairs=None, want_posterior=False):
    """Upload + run + download.  Same argument meaning as `oracle.posterior_batch` (tests compare them).
    `want_posterior`: a 4th result, the [W x k x k] matrices the windows factorised (`Batch.keep_posterior`)."""
    dev = device or default_device()
    W = len(start) if start is not None else len(row_idx)
    b = Batch(dev, strategy, k, N, n_r, gamma, W, m or 0, flags)
    try:
        if rhs is not None:
            b.set_rhs(rhs)
        if shift is not None:
            b.set_shift(shift)
        b.upload(panel, start=start, hf_panel=hf_panel, hf_start=hf_start, w0=w0, n0=n0, row_idx=row_idx,
                 n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj, hf_row_idx=hf_row_idx, hf_count=hf_count,
                 ret_pairs=ret_pairs, hf_ret_pairs=hf_ret_pairs)
        if want_posterior:
            b.keep_posterior()
        b.run()
        if want_posterior:
            return (*b.download(want_aux=want_aux), b.download_posterior())
        return b.download(want_aux=want_aux)
    finally:
        b.close()
