"""The condition that keeps tests/test_gpu_run_options.py honest, checked without a GPU: for every case the helper generates
(size, layout, option set) the oracle's result and an independent fp64 solve of the same system - scipy's Cholesky on the
matrix assembled from the oracle's own T, t, S0 - differ by no more than ONE TENTH of the bound the GPU test applies.  A case
that misses it gets more rows, never a wider bound."""
import numpy as np
import pytest

import _run_option_cases as cases

MARGIN = 0.1


@pytest.fixture(autouse=True)
def one_blas_thread():
    with cases.small_matrix_blas():
        yield


def ratio_to_bound(ref, other, what):
    """max |ref - other| over the bound of the GPU test; printed, then held below MARGIN."""
    bound = cases.sol_bound(ref)
    err = float(np.abs(ref - other).max())
    print(f"{what}: |oracle - cholesky| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3e}")
    assert np.isfinite(other).all() and np.isfinite(ref).all()
    assert err <= MARGIN * bound, f"{what}: {err:.3e} > {MARGIN} x {bound:.3e}"
    return err / bound


def check_jeffreys(k, W):
    worst = 0.0
    for layout in cases.LAYOUTS:
        case = cases.make_case("jeffreys", k, layout, W)
        if layout == "index":
            assert (case["upload"]["n_rows"] < case["n_r"]).any()
        plain = {}
        for flag in cases.FLAGS:
            for name, shifted, with_rhs in cases.JEFFREYS_RUNS:
                ref = cases.jeffreys_reference(case, flag, shifted, with_rhs)
                plain[flag] = ref if name == "plain" else plain[flag]
                worst = max(worst, ratio_to_bound(ref, cases.independent_jeffreys(case, flag, shifted, with_rhs),
                                                  f"jeffreys k={k} {layout} flag={flag} {name}"))
        # the row-count centring must show: fewer rows than N in every window
        apart = float(np.abs(plain[0] - plain[cases.FLAG_CENTER_BY_ROWS]).max())
        scale = max(1.0, float(np.abs(plain[0]).max()))
        print(f"jeffreys k={k} {layout}: default vs row-count centring {apart:.3e} apart")
        if layout == "index":
            assert apart > cases.DISCRIMINATE * scale
    return worst


def check_conjugate(k, W):
    worst = 0.0
    for layout in cases.LAYOUTS:
        case = cases.make_case("conjugate", k, layout, W)
        ref, ind = cases.conjugate_reference(case), cases.independent_conjugate(case)
        assert (ref["aux"][:, 5] > 0).all() and (ref["aux_rhs"][:, 5] > 0).all()       # n1 - w1'S1 w1: status OK in both runs
        for key in ("weights", "weights_rhs"):
            worst = max(worst, ratio_to_bound(ref[key], ind[key], f"conjugate k={k} {layout} {key}"))
        for key in ("aux", "aux_rhs"):
            tol = cases.AUX_TOL
            err = np.abs(ref[key] - ind[key]) / (tol["atol"] + tol["rtol"] * np.abs(ref[key]))
            print(f"conjugate k={k} {layout} {key}: worst ratio to the aux bound {err.max():.3e}")
            assert err.max() <= MARGIN
            worst = max(worst, float(err.max()))
    return worst


@pytest.mark.parametrize("nt", cases.TILE_COUNTS)
def test_jeffreys_cases_of_the_register_tile_path_are_well_posed(nt):
    worst = max(check_jeffreys(k, 4) for k in cases.sizes_of_tile_count(nt))
    print(f"NT={nt}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("nt", cases.TILE_COUNTS)
def test_conjugate_cases_of_the_register_tile_path_are_well_posed(nt):
    worst = max(check_conjugate(k, 3) for k in cases.border_sizes_of_tile_count(nt))
    print(f"NT={nt}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("k", cases.TILED_SIZES)
def test_cases_of_the_tiled_path_are_well_posed(k):
    worst = max(check_jeffreys(k, 3), check_conjugate(k, 3))
    print(f"k={k}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("k", cases.PORTFOLIO_SIZES)
def test_portfolio_cases_are_well_posed(k):
    """Jorion: _jorion_from_solves on Cholesky solves against oracle.jorion_window.  Greyserman: the stand-in on
    numpy.linalg.solve (the GPU test's reference) against the same algebra on Cholesky solves."""
    case, kw, draws = cases.portfolio_case(k)
    assert kw["start"] is None and (kw["n_rows"] < case["n_r"]).any()
    ratio_to_bound(cases.jorion_reference(case), cases.jorion_from(case, cases._cholesky_solve), f"jorion k={k}")
    ratio_to_bound(cases.greyserman_from(case, draws), cases.greyserman_from(case, draws, cases._cholesky_solve),
                   f"greyserman k={k}")
