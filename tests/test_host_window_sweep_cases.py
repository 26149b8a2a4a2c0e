"""Window sweep, what can be checked without a GPU about the case table (tests/_window_sweep_cases.py): for every (case,
window, length) the GPU test compares, the oracle's conjugate_window / jeffreys_window and an independent np.longdouble Cholesky
solve of the same system agree within a QUARTER of the bound the GPU test applies - so a miss on the GPU is the kernel's, not
the reference's.  No pair is skipped.  Also: the reference of the GPU test (oracle.posterior_batch on the suffix) is that same
oracle call, and the table has the shapes it is there for."""
import numpy as np
import pytest

from oracle import oracle

import _window_sweep_cases as cases

LD = np.longdouble


def chol_solve(A, b):
    """A x = b by Cholesky in extended precision (A symmetric positive definite, np.longdouble)."""
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    A = A.copy()
    for j in range(n):
        d = np.sqrt(A[j, j])
        Lm[j:, j] = A[j:, j] / d
        A[j + 1:, j + 1:] -= np.outer(Lm[j + 1:, j], Lm[j + 1:, j])
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - Lm[i, :i] @ y[:i]) / Lm[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - Lm[i + 1:, i] @ x[i + 1:]) / Lm[i, i]
    return x


def conjugate_ld(X, Y, w0, n0, N, k, gamma):
    """ref:819-836 in np.longdouble -> (weights, aux[:6])."""
    X, Y, w0, n0 = X.astype(LD), Y.astype(LD), w0.astype(LD), LD(n0)
    m = Y.shape[0]
    Yc = Y - Y.mean(axis=0)
    S0 = n0 * ((Yc.T @ Yc) / LD(m - 1) * LD(m))
    T, t = X.T @ X, X.sum(axis=0)
    q0 = w0 @ (S0 @ w0)
    a = n0 + k + 2
    c = 2 * n0 / (a + np.sqrt(a * a + 4 * n0 * q0))
    S1 = S0 + T
    w1 = chol_solve(S1, c * (S0 @ w0) + t)
    n1 = n0 + N
    q1 = w1 @ (S1 @ w1)
    wts = (n1 + k + 2) * w1 / (n1 - q1) / LD(gamma)
    return wts, np.array([n0, n1, c, q0, q1, n1 - q1], dtype=LD)


def jeffreys_ld(X, N, gamma):
    """ref:600-606, 849 in np.longdouble; N = None: no t t'/N term.  -> (weights, q1 = t'M^-1 t)."""
    X = X.astype(LD)
    T, t = X.T @ X, X.sum(axis=0)
    J = T - np.outer(t, t) / LD(N) if N is not None else T
    x = chol_solve(J, t)
    return x / LD(gamma), t @ x


def quarter(got, ref, what):
    b = cases.bound(ref)
    err = float(np.abs(got - ref.astype(LD)).max())
    assert np.isfinite(ref).all() and err <= 0.25 * b, f"{what}: {err:.3e} > a quarter of {b:.3e}"
    return err / b


CONJ = list(cases.problems("conjugate"))
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
            for p in range(cases.P):
                wt, a = oracle.conjugate_window(X, Y, pr["w0"][w, p], float(pr["n0"][w, p, l]), int(pr["N"][l]), pr["k"], cases.GAMMA,
                                                return_aux=True)
                assert np.array_equal(wt, ref[w, p, l])                # the GPU test's reference is this oracle call
                ld, ald = conjugate_ld(X, Y, pr["w0"][w, p], pr["n0"][w, p, l], int(pr["N"][l]), pr["k"], cases.GAMMA)
                worst = max(worst, quarter(ld, wt, f"{pr['id']} w={w} p={p} rows={pr['rows'][w, l]}"))
                # aux[:6] against the extended-precision values, in units of the GPU test's tolerance
                ra = np.abs(raux[w, p, l, :6].astype(LD) - ald) / (cases.AUX_ATOL + cases.AUX_RTOL * np.abs(ald))
                worst_aux = max(worst_aux, float(ra.max()))
                assert raux[w, p, l, 5] > 0                            # no BAD_DENOM among the cases
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
            wt = oracle.jeffreys_window(X, Nw, cases.GAMMA)
            assert np.array_equal(wt, ref[w, 0, l])
            ld, q1_ld = jeffreys_ld(X, Nw, cases.GAMMA)
            worst = max(worst, quarter(ld, wt, f"{pr['id']} flag={flag} w={w} rows={pr['rows'][w, l]}"))
            # the GPU test's stand-in for q1, gamma t'(the oracle's weights), in units of its tolerance for aux
            q1 = cases.GAMMA * X.sum(axis=0) @ wt
            worst_q1 = max(worst_q1, float(abs(LD(q1) - q1_ld) / (cases.AUX_ATOL + cases.AUX_RTOL * abs(q1_ld))))
    print(f"{pr['id']} flag={flag}: worst |oracle - longdouble| = {worst:.2e} of the bound, q1 stand-in {worst_q1:.2e} of its tolerance")
    assert worst_q1 <= 0.25


def test_the_table_covers_what_it_is_there_for():
    assert sorted((k + 1 + 15) // 16 for k in cases.CASES) == [1, 3, 9]
    for k, (N, conj, jeff) in cases.CASES.items():
        for rows0 in conj + jeff:
            assert rows0 == sorted(set(rows0)) and rows0[-1] == N - 1 and len(rows0) <= 16
        assert all(r > k for rows0 in jeff for r in rows0)
    assert len(cases.LIST16_143) == 16
    seg = lambda rows0: set(np.diff([0] + rows0).tolist())
    assert {1, 2, 3, 5} <= seg(cases.CASES[5][1][0]) | seg(cases.CASES[33][1][0])
    assert {1, 2, 3, 5} <= seg(cases.LIST16_143)
    ends = {r % 4 for r in cases.CASES[33][1][0]} | {r % 64 for r in cases.CASES[33][1][0]}
    assert {0, 1, 3, 63} <= ends                                       # on, before and after a multiple of 4 and of 64
    # a tie: window 1 shifts a count onto its neighbour
    tied = cases.rows_table(cases.CASES[33][1][0], [129, 129])
    assert tied[0].tolist() == cases.CASES[33][1][0] and tied[1, 0] == tied[1, 1] == 1
    # the index layout cuts the longest length to the window's own rows
    assert any((pr["rows"][:, -1] < pr["inp"]["n_r"]).any() for pr in cases.problems("conjugate", ks=[5]) if pr["layout"] == "index")
