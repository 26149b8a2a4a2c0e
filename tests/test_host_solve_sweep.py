"""Solve sweeps without a GPU: the symbols exist, NULL batches are refused, and the sweep kernel's range is declared."""
import ctypes

from incorporating_different_sources_amd import _native

SYMBOLS = ("tp_sweep_max_assets", "tp_batch_solve_sweep", "tp_batch_download_sweep")


def test_symbols_are_listed_and_exported():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS + ("tp_batch_download_sweep_rhs",):
        assert name in _native.EXPORTS
        assert hasattr(lib, name), f"libtangency.so does not export {name}"


def test_null_batch_is_invalid():
    lib = _native.lib
    assert lib.tp_batch_solve_sweep(None, 0, None, 0, None, 1) == _native.TP_ERR_INVALID
    assert lib.tp_batch_download_sweep(None, None, None) == _native.TP_ERR_INVALID
    assert lib.tp_batch_download_sweep_rhs(None, None) == _native.TP_ERR_INVALID


def test_sweep_range():
    assert 143 <= _native.sweep_max_assets() <= _native.max_assets()
    assert _native.SWEEP_MAX_RHS == 16


def test_solve_sweep_checks_shapes_before_the_library_is_called():
    """Shape errors are ValueErrors raised by the binding itself (a Batch needs a device, so the checks are exercised on
    an object that has none: reaching the library would fail differently)."""
    import numpy as np
    import pytest

    class NoLibrary(_native.Batch):
        def __init__(self, W, k):
            self.W, self.k, self._b, self.dev = W, k, None, None

        def __del__(self):
            pass

    b = NoLibrary(4, 6)
    for kw in (dict(shift=np.zeros((4, 3))), dict(shift=np.zeros((5, 3, 2))), dict(shift=np.zeros((4, 0, 2))),
               dict(rhs=np.zeros((4, 2, 7))), dict(rhs=np.zeros((3, 2, 6))), dict(rhs=np.zeros((4, 16, 6))),
               dict(default_rhs=False), dict(out=(np.empty((4, 1, 2, 6)), np.empty((4, 1), dtype=np.int32))),
               dict(out=(np.empty((4, 1, 1, 6)), np.empty((4, 1), dtype=np.int64)))):
        with pytest.raises(ValueError):
            b.solve_sweep(**kw)
