"""CPU check behind tests/test_gpu_prior_sweep_tiled.py: on every shape of the oracle-parity and
hf_count tests, (1) the oracle returns status 0 for every (window, prior), and (2) the weights from the raw-moment centred
scatter C = Y'Y - (Y'1)(Y'1)'/m that the tiled prior sweep forms differ from those of the two-pass form
sum (y - ybar)(y - ybar)' by far less than the tests' tolerance.  Both forms in numpy float64, the same solve for both.

    python tools/prior_sweep_tiled_centring.py > profiles/r09_prior_sweep_tiled_centring.txt
"""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from incorporating_different_sources_amd import synthetic  # noqa: E402


def test_helpers():
    """The shapes, priors, layouts and oracle loop of tests/test_gpu_prior_sweep_tiled.py, so that this check runs on exactly what
    the tests run on.  NB: that module imports the package's native binding, so the library must be built (no GPU is needed:
    nothing here creates a device); the functions below take the helpers as an argument and depend on numpy alone."""
    spec = importlib.util.spec_from_file_location("t", os.path.join(REPO, "tests", "test_gpu_prior_sweep_tiled.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


def window_rows(panel, kw, w, k, n_r, m):
    cols = kw["col_idx"][w] if kw.get("col_idx") is not None else np.arange(k)
    nr = int(kw["n_rows"][w]) if kw.get("n_rows") is not None else n_r
    rows = kw["row_idx"][w][:nr] if kw.get("row_idx") is not None else kw["start"][w] + np.arange(nr)
    X = panel[np.ix_(rows, cols)]
    if kw.get("rf_adj") is not None:
        X = X - kw["rf_adj"][w][:nr, None]
    mm = int(kw["hf_count"][w]) if kw.get("hf_count") is not None else m
    hrows = kw["hf_row_idx"][w][:mm] if kw.get("hf_row_idx") is not None else kw["hf_start"][w] + np.arange(mm)
    return X, kw["hf_panel"][np.ix_(hrows, cols)]


def weights(C, T, tt, n0, w0, mm, k, N, gamma):
    a = n0 * (mm / (mm - 1.0))
    v = a * (C @ w0)
    q0 = w0 @ v
    g = n0 + k + 2
    c = 2 * n0 / (g + np.sqrt(g * g + 4 * n0 * q0))
    S1 = a * C + T
    w1 = np.linalg.solve(S1, c * v + tt)
    n1 = n0 + N
    return (n1 + k + 2) * w1 / (n1 - w1 @ S1 @ w1) / gamma


def main(t):
    cases = [(k, N, 2, 4, 890000 + k, ("contiguous", "index"), False) for k, N in t.SHAPES]
    cases.append((150, 200, 2, 4, 890000 + 150, ("index+hf",), True))
    print("shape layout: max|w_raw - w_twopass|, its ratio to the test bound 1e-10 max(1, |ref|.max()), max|w_twopass - oracle|, "
          "intraday |mean| / std")
    worst = 0.0
    for k, N, W, P, seed, which, hfi in cases:
        inp = synthetic.make_kernel_inputs(k, N, W, seed=seed)
        n0, w0 = t.make_priors(np.random.default_rng(seed), W, P, k, N)
        for name, panel, ukw, okw in t.layouts(inp, seed, hfi):
            if name not in which:
                continue
            ref, _ = t.oracle_sweep(k, N, panel, okw, n0, w0)          # asserts status 0 for every (window, prior)
            bound = t.TOL * max(1.0, float(np.abs(ref).max()))
            d = e = off = 0.0
            for w in range(W):
                X, Y = window_rows(panel, ukw, w, k, inp["n_r"], inp["m"])
                mm = Y.shape[0]
                T, tt = X.T @ X, X.sum(axis=0)
                Yc = Y - Y.mean(axis=0)
                C2 = Yc.T @ Yc
                s = Y.sum(axis=0)
                Cr = Y.T @ Y - np.outer(s, s) / mm
                off = max(off, float(np.abs(Y.mean(axis=0)).max() / Y.std(axis=0).min()))
                for p in range(P):
                    wr = weights(Cr, T, tt, n0[w, p], w0[w, p], mm, k, N, t.GAMMA)
                    w2 = weights(C2, T, tt, n0[w, p], w0[w, p], mm, k, N, t.GAMMA)
                    d = max(d, float(np.abs(wr - w2).max()))
                    e = max(e, float(np.abs(w2 - ref[w, p]).max()))
            worst = max(worst, d / bound)
            print(f"k={k} N={N} {name}: {d:.3e}  {d / bound:.3e}  {e:.3e}  {off:.2f}   oracle status 0 for all {W * P} pairs")
    print(f"worst ratio to the bound: {worst:.3e} (required: <= 1e-2)")
    assert worst <= 1e-2


if __name__ == "__main__":
    main(test_helpers())
