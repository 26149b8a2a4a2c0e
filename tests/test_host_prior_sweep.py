"""Prior sweep, what can be checked without a GPU: the C-ABI symbols, the binding's argument checks (before any device call)
and the spec-list check of calculate_weights_for_specs(share_grams=True)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from incorporating_different_sources_amd import _native

SYMBOLS = ("tp_batch_prior_sweep", "tp_batch_download_prior_sweep")


def test_prior_sweep_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "tangency_posterior.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"libtangency.so does not export {name}"
        assert name in _native.EXPORTS


class _NoDevice:
    """Stands in for the device and the library handle: any call into the library fails the test."""
    def _check(self, rc):
        pytest.fail("the binding called into the library")


def _batch(W=3, k=4):
    b = object.__new__(_native.Batch)
    b.dev, b.W, b.k, b._b = _NoDevice(), W, k, ctypes.c_void_p()
    return b


@pytest.mark.parametrize("n0,w0", [
    (np.ones((3,)), np.ones((3, 1, 4))),                   # n0 not [W x P]
    (np.ones((2, 2)), np.ones((2, 2, 4))),                 # wrong W
    (np.ones((3, 0)), np.ones((3, 0, 4))),                 # P = 0
    (np.ones((3, 2)), np.ones((3, 2, 5))),                 # wrong k
    (np.ones((3, 2)), np.ones((3, 3, 4))),                 # P of w0 differs
    (np.ones((3, 2)), np.ones((3, 2))),                    # w0 not 3-D
    (np.ones((3, 2), dtype=complex), np.ones((3, 2, 4))),  # dtypes that are not real numbers
    (np.ones((3, 2)), np.full((3, 2, 4), "x")),
    (np.ones((3, 2)), np.full((3, 2, 4), None, dtype=object)),
    (None, np.ones((3, 2, 4))),
    (np.ones((3, 2)), None),
])
def test_binding_rejects_wrong_shapes_and_dtypes_before_any_device_call(n0, w0, monkeypatch):
    monkeypatch.setattr(_native.lib, "tp_batch_prior_sweep", lambda *a: pytest.fail("the binding called into the library"), raising=False)
    with pytest.raises(ValueError):
        _batch().prior_sweep(n0, w0)


def test_share_grams_refuses_the_spec_lists_the_default_refuses():
    from incorporating_different_sources_amd import portfolio_calculations as pc

    def spec(strat, k=5):
        return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": "daily",
                "rolling_window": 30, "rolling_window_frequency": "daily", "mcm_scaling": 1, "display_name": strat}

    for specs in ([spec("conjugate_hf_vix_vw"), spec("jeffreys")],                       # a non-conjugate spec
                  [spec("conjugate_hf_vix_vw"), spec("conjugate_hf_vix_ew", k=6)]):      # two families
        errors = []
        for share in (False, True):
            with pytest.raises(ValueError) as e:
                pc.calculate_weights_for_specs([], specs, {}, share_grams=share)
            errors.append(str(e.value))
        assert errors[0] == errors[1]
    assert pc.calculate_weights_for_specs([], [], {}, share_grams=True) == []
