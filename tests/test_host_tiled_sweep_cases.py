"""The condition that keeps tests/test_gpu_tiled_sweeps_large.py honest, checked without a GPU: for every case of
tests/_tiled_sweep_cases.py the reference (numpy.linalg.solve on the oracle's statistics, or the oracle itself) and an
independent fp64 solve of the same system - scipy's Cholesky on the same matrix, the conjugate nu rescale redone from its w1 -
differ by no more than ONE TENTH of the bound the GPU test applies; every reference status is OK (finite weights, a positive
conjugate denominator).  A case that misses it gets another seed, more rows or another scaling, never a wider bound.

Worst |LU - Cholesky| over the GPU test's bound, per group, as measured on the CPU (the whole file takes about half a minute):
    Jeffreys solve sweep   1.1e-3  (k = 2046; 3.2e-4 .. 5.8e-4 up to k = 1023), |ref|.max() 3 .. 21
    conjugate solve sweep  3.3e-4  (k = 640)
    prior sweep, weights   2.8e-2  (k = 2047; 1.1e-2 at k = 1023, <= 5.2e-3 below)
    prior sweep, aux       5.1e-2  (q1 at k = 1023, the one case on the 0.001 scaling; <= 2.0e-2 elsewhere)
    denom / n1 >= 0.063 (k = 2047), so every conjugate status is OK with room to spare."""
import numpy as np
import pytest

import _tiled_sweep_cases as cases

MARGIN = 0.1


def ratio_to_bound(ref, other, what):
    """max |ref - other| over the bound of the GPU test; printed, then held below MARGIN."""
    bound = cases.sol_bound(ref)
    err = float(np.abs(ref - other).max())
    print(f"{what}: |lu - cholesky| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3e}, |ref|.max() = {np.abs(ref).max():.3e}")
    assert np.isfinite(other).all() and np.isfinite(ref).all()
    assert err <= MARGIN * bound, f"{what}: {err:.3e} > {MARGIN} x {bound:.3e}"
    return err / bound


@pytest.mark.parametrize("k,R,layouts", cases.JEFFREYS_SOLVE, ids=[cases.case_id(c) for c in cases.JEFFREYS_SOLVE])
def test_jeffreys_solve_sweep_cases_are_well_posed(k, R, layouts):
    worst = 0.0
    for layout in layouts:
        for no_center in (False, True):
            ref = cases.jeffreys_solve_reference(k, R, layout, no_center, independent=True)
            worst = max(worst, ratio_to_bound(ref["x"], ref["x_ind"], f"jeffreys k={k} R={R} {layout} no_center={no_center}"))
    print(f"jeffreys solve sweep k={k} R={R}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("k,N,hf_days,R", cases.CONJUGATE_SOLVE, ids=[cases.case_id(c) for c in cases.CONJUGATE_SOLVE])
def test_conjugate_solve_sweep_cases_are_well_posed(k, N, hf_days, R):
    ref = cases.conjugate_solve_reference(k, N, hf_days, R, independent=True)
    worst = ratio_to_bound(ref["x"], ref["x_ind"], f"conjugate k={k} N={N} hf_days={hf_days} R={R}")
    print(f"conjugate solve sweep k={k}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("k,N,hf_days,layouts", cases.PRIOR, ids=[cases.case_id(c) for c in cases.PRIOR])
def test_prior_sweep_cases_are_well_posed(k, N, hf_days, layouts):
    worst = worst_aux = 0.0
    for layout in layouts:
        c = cases.prior_case(k, N, hf_days, layout)
        assert (c["m"] - 1) + (c["n_r"] - 1) > k                                    # S1 = S0 + T can have full rank
        if layout == "index+hf":
            assert len(set(c["upload"]["hf_count"])) == cases.W and (c["upload"]["hf_count"] < c["m"]).all()
        ref = cases.prior_reference(k, N, hf_days, layout, independent=True)
        assert (ref["aux"][..., 5] > 0).all() and (ref["aux_ind"][..., 5] > 0).all()    # n1 - w1'S1 w1: TP_STATUS_OK
        what = f"prior k={k} N={N} hf_days={hf_days} {layout}"
        worst = max(worst, ratio_to_bound(ref["weights"], ref["weights_ind"], what))
        ratio = cases.aux_ratio(ref["aux_ind"], ref["aux"])
        print(f"{what}: aux, worst ratio to its bound {ratio:.3e}; denom / n1 >= {(ref['aux'][..., 5] / ref['aux'][..., 1]).min():.3f}")
        assert ratio <= MARGIN
        worst_aux = max(worst_aux, ratio)
    print(f"prior sweep k={k}: worst ratio {worst:.3e} (weights), {worst_aux:.3e} (aux)")
