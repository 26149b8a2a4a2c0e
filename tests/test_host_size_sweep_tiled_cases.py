"""Tiled size sweep, what can be checked without a GPU: that the cases of tests/_size_sweep_tiled_cases.py are well-posed - the
oracle reference and an independent Cholesky solve of the same prefix system agree within a TENTH of the bound the GPU test
applies, so a miss on the GPU is the kernel's -, the binding's argument checks (before any device call), and the routing of
calculate_weights_for_sizes with the switch off (unchanged) and on."""
import ctypes

import numpy as np
import pytest

from incorporating_different_sources_amd import _native, batch

import _size_sweep_tiled_cases as cases

CONJ = [(n, lay) for n in cases.CONJUGATE_CASES for lay in cases.layouts_of(n)]
JEFF = [(n, lay, f) for n in cases.JEFFREYS_CASES for lay in cases.layouts_of(n)
        for f in (cases.JEFFREYS_N if n in cases.ALL_FLAGS_CASES else (0,))]


def _tenth(got, ref, what):
    bound = cases.sol_bound(ref)
    err = float(np.abs(got - ref).max())
    print(f"{what}: max|cholesky - oracle| = {err:.3e} = {err / bound:.2e} of the bound {bound:.3e}")
    assert np.isfinite(ref).all() and err <= 0.1 * bound, f"{what}: {err:.3e} > a tenth of {bound:.3e}"


@pytest.mark.parametrize("name,layout", CONJ, ids=[f"{n}-{lay}" for n, lay in CONJ])
def test_conjugate_references_are_good_to_a_tenth_of_the_bound(name, layout):
    c = cases.case(name, "conjugate", layout)
    r = cases.conjugate_reference(name, layout, independent=True)
    for s, ks in enumerate(c["sizes"]):
        _tenth(r["weights_ind"][:, :, s], r["weights"][:, :, s], f"conjugate {name} {layout} k_s={ks}")
        assert not r["weights"][:, :, s, ks:].any()
        assert (r["aux"][:, :, s, 5] > 0).all()                        # no BAD_DENOM among the cases
    ratio = cases.aux_ratio(r["aux_ind"], r["aux"])
    print(f"conjugate {name} {layout}: aux |cholesky - oracle| = {ratio:.2e} of AUX_TOL")
    assert ratio <= 0.1


@pytest.mark.parametrize("name,layout,flag", JEFF, ids=[f"{n}-{lay}-{f}" for n, lay, f in JEFF])
def test_jeffreys_references_are_good_to_a_tenth_of_the_bound(name, layout, flag):
    c = cases.case(name, "jeffreys", layout)
    r = cases.jeffreys_reference(name, layout, flag, independent=True)
    for s, ks in enumerate(c["sizes"]):
        _tenth(r["weights_ind"][:, :, s], r["weights"][:, :, s], f"jeffreys {name} {layout} flag={flag} k_s={ks}")


def test_case_geometry_is_what_the_cases_are_there_for():
    """(NSB, NS) per case, and where the right-hand-side columns fall."""
    geo = {n: ((k + 63) // 64, (k + len(sz) + 63) // 64) for n, (k, N, hf, sz) in cases.CASES.items()}
    assert geo == {"A": (3, 3), "B": (3, 4), "C": (3, 4), "D": (4, 5), "E": (9, 9), "F": (32, 32)}
    for n, (k, N, hf, sz) in cases.CASES.items():
        assert N == 2 * k + 24 and list(sz) == sorted(set(sz)) and sz[-1] == k and len(sz) <= _native.SWEEP_MAX_RHS
    kB, kC, kD, kF = (cases.CASES[n][0] for n in "BCDF")
    assert kB % 64 == 63 and kB // 64 == 2                              # B: right-hand-side column k closes super-tile 2
    assert kC % 64 == 0                                                 # C: the right-hand sides open a super-tile of their own
    assert kD // 64 == 3 and (kD + 15) // 64 == 4                      # D: columns k .. k+15 straddle super-tiles 3 and 4
    assert kF + len(cases.CASES["F"][3]) == 2048


# ---- the binding ------------------------------------------------------------------------------------------------------
class _NoDevice:
    def _check(self, rc):
        pytest.fail("the binding called into the library")


def _batch(W=3, k=200):
    b = object.__new__(_native.Batch)
    b.dev, b.W, b.k, b._b = _NoDevice(), W, k, ctypes.c_void_p()
    return b


@pytest.mark.parametrize("sizes,n0,w0", [
    ([], np.ones((3, 2)), np.ones((3, 2, 0, 200))),                    # no size
    (list(range(1, 18)), None, None),                                  # more than 16 sizes
    ([0, 150], np.ones((3, 2)), np.ones((3, 2, 2, 200))),              # below 1
    ([150, 201], np.ones((3, 2)), np.ones((3, 2, 2, 200))),            # above k
    ([150, 150], np.ones((3, 2)), np.ones((3, 2, 2, 200))),            # not strictly increasing
    ([[100, 200]], np.ones((3, 2)), np.ones((3, 2, 2, 200))),          # not 1-D
    ([100.0, 200.0], np.ones((3, 2)), np.ones((3, 2, 2, 200))),        # not integers
    (None, np.ones((3, 2)), np.ones((3, 2, 2, 200))),
    ([100, 200], np.ones((3,)), np.ones((3, 1, 2, 200))),              # n0 not [W x P]
    ([100, 200], np.ones((2, 2)), np.ones((2, 2, 2, 200))),            # wrong W
    ([100, 200], np.ones((3, 2)), np.ones((3, 2, 2, 199))),            # wrong k
    ([100, 200], np.ones((3, 2)), np.ones((3, 2, 3, 200))),            # S of w0 differs
    ([100, 200], np.ones((3, 2), dtype=complex), np.ones((3, 2, 2, 200))),
    ([100, 200], None, np.ones((3, 2, 2, 200))),                       # one of the two priors alone
    ([100, 200], np.ones((3, 2)), None),
])
def test_binding_rejects_wrong_arguments_before_any_device_call(sizes, n0, w0, monkeypatch):
    monkeypatch.setattr(_native.lib, "tp_batch_size_sweep_tiled", lambda *a: pytest.fail("the binding called into the library"), raising=False)
    with pytest.raises(ValueError):
        _batch().size_sweep_tiled(sizes, n0, w0)


def test_symbol_is_exported_by_the_library_and_listed():
    assert "tp_batch_size_sweep_tiled" in _native.EXPORTS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "tp_batch_size_sweep_tiled")


# ---- the routing of calculate_weights_for_sizes -------------------------------------------------------------------------
def _spec(k, strat="conjugate_hf_vix_vw"):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": "daily",
            "rolling_window": 30, "rolling_window_frequency": "daily", "mcm_scaling": 1, "display_name": f"{strat}_{k}"}


def _routed(monkeypatch, sizes):
    """(sizes the nested pack was asked for, sizes that went through _weights_for_dates); the pack raises, so nothing is swept
    and no device is needed."""
    from incorporating_different_sources_amd import portfolio_calculations as pc
    packs, alone = [], []

    def pack(dates, spec, sz, md, **kw):
        packs.append(list(sz))
        raise ValueError("no pack in this test")

    monkeypatch.setattr(batch, "pack_windows_nested", pack)
    monkeypatch.setattr(pc, "_weights_for_dates", lambda d, sp, m: (alone.append(sp["size"]), (np.zeros((len(d), sp["size"])), [], None, None))[1])
    monkeypatch.setattr(pc, "_fill_spec_cache", lambda sps, d, m, w, n, same, lab, cols, cp: [(w, lab, cols, cp)])
    monkeypatch.setattr(_native, "Batch", lambda *a, **kw: pytest.fail("a device batch was created"))
    out = pc.calculate_weights_for_sizes([], [_spec(k) for k in sizes], {"members_of": None})
    assert [r[0].shape[1] for r in out] == list(sizes)
    return packs, alone


def test_routing_is_unchanged_with_the_switch_off(monkeypatch):
    from incorporating_different_sources_amd import portfolio_calculations as pc
    assert getattr(pc, "SIZE_SWEEP_TILED", False) is False             # off by default
    smax = _native.sweep_max_assets()
    packs, alone = _routed(monkeypatch, [100, smax, smax + 1, 150])
    assert packs == [[100, smax]]                                      # the sweep is asked for the sizes it serves only
    assert alone == [100, smax, smax + 1, 150]                         # (the pack raised: every spec on its own)
    packs, alone = _routed(monkeypatch, [150, 200])
    assert packs == [] and alone == [150, 200]                         # above the bound: _weights_for_dates, no pack


def test_switch_on_packs_every_size_once_at_the_largest(monkeypatch):
    from incorporating_different_sources_amd import portfolio_calculations as pc
    monkeypatch.setattr(pc, "SIZE_SWEEP_TILED", True)
    smax = _native.sweep_max_assets()
    assert _routed(monkeypatch, [100, smax + 1, 150])[0] == [[100, smax + 1, 150]]
    assert _routed(monkeypatch, [100, smax])[0] == [[100, smax]]       # largest size within the LDS sweep: as with the switch off
    # what one tiled sweep cannot hold keeps the old route: more than SWEEP_MAX_RHS sizes, k + S beyond the arena side
    many = list(range(130, 130 + _native.SWEEP_MAX_RHS + 1))
    assert _routed(monkeypatch, many)[0] == [[ks for ks in many if ks <= smax]]
    assert _routed(monkeypatch, [100, _native.max_assets()])[0] == [[100]]
