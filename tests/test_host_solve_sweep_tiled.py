"""Solve sweeps above sweep_max_assets() without a GPU: the symbol exists, a NULL batch is refused, and the binding checks
shapes before the library is called."""
import ctypes

import numpy as np
import pytest

from incorporating_different_sources_amd import _native


def test_symbol_is_listed_and_exported():
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert "tp_batch_solve_sweep_tiled" in _native.EXPORTS
    assert hasattr(lib, "tp_batch_solve_sweep_tiled"), "libtangency.so does not export tp_batch_solve_sweep_tiled"


def test_null_batch_is_invalid():
    assert _native.lib.tp_batch_solve_sweep_tiled(None, 0, None, 0, None, 1) == _native.TP_ERR_INVALID


def test_solve_sweep_tiled_checks_shapes_before_the_library_is_called():
    """Shape errors are ValueErrors raised by the binding itself (a Batch needs a device, so the checks are exercised on
    an object that has none: reaching the library would fail differently)."""

    class NoLibrary(_native.Batch):
        def __init__(self, W, k):
            self.W, self.k, self._b, self.dev = W, k, None, None

        def __del__(self):
            pass

    b = NoLibrary(4, 150)
    for kw in (dict(shift=np.zeros((4, 3))), dict(shift=np.zeros((5, 3, 2))), dict(shift=np.zeros((4, 0, 2))),
               dict(rhs=np.zeros((4, 2, 151))), dict(rhs=np.zeros((3, 2, 150))), dict(rhs=np.zeros((4, 16, 150))),
               dict(default_rhs=False), dict(out=(np.empty((4, 1, 2, 150)), np.empty((4, 1), dtype=np.int32))),
               dict(out=(np.empty((4, 1, 1, 150)), np.empty((4, 1), dtype=np.int64)))):
        with pytest.raises(ValueError):
            b.solve_sweep_tiled(**kw)
