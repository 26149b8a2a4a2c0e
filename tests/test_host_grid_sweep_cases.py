"""Grid sweep, what can be checked without a GPU about the case table (tests/_grid_sweep_cases.py): for every (case, window,
length, size) the GPU test compares, the oracle's conjugate_window / jeffreys_window on the suffix rows and prefix columns and
an independent np.longdouble Cholesky solve of the same system agree within a QUARTER of the bound the GPU test applies - so a
miss on the GPU is the kernel's, not the reference's.  No entry is skipped.  Also: the reference of the GPU test
(oracle.posterior_batch on the suffix and the prefix) is that same oracle call, and the table has the shapes it is there for."""
import numpy as np
import pytest

from oracle import oracle

import _grid_sweep_cases as cases
from test_host_window_sweep_cases import LD, conjugate_ld, jeffreys_ld, quarter

CONJ = cases.problems("conjugate")
JEFF = [(pr, f) for pr in cases.problems("jeffreys") for f in cases.JEFFREYS_FLAGS]


@pytest.mark.parametrize("pr", CONJ, ids=[pr["id"] for pr in CONJ])
def test_conjugate_oracle_is_good_to_a_quarter_of_the_bound(pr):
    ref, rstat, raux = cases.reference(pr)
    assert (rstat == 0).all()
    worst, worst_aux = 0.0, 0.0
    for w in range(cases.W):
        for l in range(len(pr["N"])):
            X, Y = cases.window_rows(pr, w, l)
            assert X.shape == (pr["rows"][w, l], pr["k"])
            for s, ks in enumerate(pr["sizes"]):
                Xs, Ys = np.ascontiguousarray(X[:, :ks]), np.ascontiguousarray(Y[:, :ks])      # the prefix as the oracle's driver gathers it
                for p in range(pr["P"]):
                    w0, n0, N = pr["w0g"][w, p, s, :ks], float(pr["n0"][w, p, l]), int(pr["N"][l])
                    wt, a = oracle.conjugate_window(Xs, Ys, w0, n0, N, ks, cases.GAMMA, return_aux=True)
                    assert np.array_equal(wt, ref[w, p, l, s, :ks]) and not ref[w, p, l, s, ks:].any()   # the GPU test's reference is this call
                    ld, ald = conjugate_ld(Xs, Ys, w0, n0, N, ks, cases.GAMMA)
                    worst = max(worst, quarter(ld, wt, f"{pr['id']} w={w} p={p} rows={pr['rows'][w, l]} k_s={ks}"))
                    ra = np.abs(raux[w, p, l, s, :6].astype(LD) - ald) / (cases.AUX_ATOL + cases.AUX_RTOL * np.abs(ald))
                    worst_aux = max(worst_aux, float(ra.max()))
                    assert raux[w, p, l, s, 5] > 0                     # no BAD_DENOM among the cases
    print(f"{pr['id']}: worst |oracle - longdouble| = {worst:.2e} of the bound, aux {worst_aux:.2e} of its tolerance")
    assert worst_aux <= 0.25


@pytest.mark.parametrize("pr,flag", JEFF, ids=[f"{pr['id']}-flag{f}" for pr, f in JEFF])
def test_jeffreys_oracle_is_good_to_a_quarter_of_the_bound(pr, flag):
    ref, rstat, _ = cases.reference(pr, flag)
    assert (rstat == 0).all()
    worst, worst_q1 = 0.0, 0.0
    for w in range(cases.W):
        for l in range(len(pr["N"])):
            X, _ = cases.window_rows(pr, w, l)
            Nw = None if flag == 2 else (X.shape[0] if flag == 1 else int(pr["N"][l]))
            for s, ks in enumerate(pr["sizes"]):
                Xs = np.ascontiguousarray(X[:, :ks])                   # the prefix as the oracle's driver gathers it
                wt = oracle.jeffreys_window(Xs, Nw, cases.GAMMA)
                assert np.array_equal(wt, ref[w, 0, l, s, :ks]) and not ref[w, 0, l, s, ks:].any()
                ld, q1_ld = jeffreys_ld(Xs, Nw, cases.GAMMA)
                worst = max(worst, quarter(ld, wt, f"{pr['id']} flag={flag} w={w} rows={pr['rows'][w, l]} k_s={ks}"))
                # the GPU test's stand-in for q1, gamma t'(the oracle's weights), in units of its tolerance for aux
                q1 = cases.GAMMA * Xs.sum(axis=0) @ wt
                worst_q1 = max(worst_q1, float(abs(LD(q1) - q1_ld) / (cases.AUX_ATOL + cases.AUX_RTOL * abs(q1_ld))))
    print(f"{pr['id']} flag={flag}: worst |oracle - longdouble| = {worst:.2e} of the bound, q1 stand-in {worst_q1:.2e} of its tolerance")
    assert worst_q1 <= 0.25


def test_the_table_covers_what_it_is_there_for():
    from _window_sweep_cases import CASES, LIST16_143
    assert sorted(cases.SIZES) == sorted(CASES) and sorted((k + 1 + 15) // 16 for k in cases.SIZES) == [1, 3, 9]
    for k, sizes in cases.SIZES.items():
        assert sizes == sorted(set(sizes)) and sizes[0] >= 1 and sizes[-1] == k
    assert len(cases.SIZES16_143) == 16 and cases.SIZES16_143 == sorted(set(cases.SIZES16_143)) and cases.SIZES16_143[-1] == 143
    every = set(cases.SIZES[33]) | set(cases.SIZES[143]) | set(cases.SIZES16_143)
    assert {32, 33, 64, 65, 128} <= every and {31, 63, 127, 129} <= set(cases.SIZES16_143)     # on, before and after 32 and 64 lanes
    conj, jeff = cases.problems("conjugate"), cases.problems("jeffreys")
    # every (k, layout, delta or not) of the first lists, and the 16 x 16 case once, at P = 1
    assert len(conj) == 3 * 3 * 2 + 1 and len(jeff) == 3 * 3 * 2
    big = [pr for pr in conj if len(pr["sizes"]) == 16]
    assert len(big) == 1 and big[0]["P"] == 1 and big[0]["rows0"] == LIST16_143 and len(big[0]["N"]) == 16
    assert big[0]["layout"] == "index" and big[0]["delta"] is not None and big[0]["w0g"].shape == (cases.W, 1, 16, 143)
    for pr in conj + jeff:
        assert pr["w0g"].shape == (cases.W, pr["P"], len(pr["sizes"]), pr["k"]) and pr["n0"].shape == (cases.W, pr["P"], len(pr["N"]))
        for s, ks in enumerate(pr["sizes"]):
            assert not pr["w0g"][:, :, s, ks:].any() and np.allclose(pr["w0g"][:, :, s].sum(axis=-1), 1.0)
    for pr in jeff:
        assert (pr["rows"] >= pr["k"] + 2).all()                           # rows to spare at the largest size, hence at every size
