"""Cases, references and bounds for the tiled sweeps (tp_batch_prior_sweep_tiled, tp_batch_solve_sweep_tiled) over the whole
large-k range, up to k + R = 2048, shared by tests/test_host_tiled_sweep_cases.py (CPU: are the cases well-posed?) and
tests/test_gpu_tiled_sweeps_large.py (GPU: do the kernels give the oracle's numbers?).  No tests in here.  It also holds the
helpers the sweep test files share: `layouts`, `make_priors`, `make_shift`.

Every reference is built from oracle.oracle, once per window: the solve sweeps solve (M_w + d I + e 1 1') X = B for all R
columns at once with numpy.linalg.solve (M_w from the oracle's own statistics), the prior sweep takes oracle.conjugate_window
per (window, prior).  `independent=True` solves the same systems a second time by Cholesky (scipy) on the same matrix, the
conjugate nu rescale redone from that w1: the CPU test holds the two within a tenth of the bound the GPU test applies, so a
miss on the GPU is the kernel's, not the reference's.  Cases and references are cached per process."""
import functools

import numpy as np

from incorporating_different_sources_amd import synthetic
from oracle import oracle

from _run_option_cases import AUX_TOL, FLAG_NO_CENTER, GAMMA, RHS_TOL, SOL_TOL, _cholesky_solve, sol_bound  # noqa: F401

W = 2
S = 3                                   # shifts per window of the Jeffreys solve sweep
P = 4                                   # priors per window of the prior sweep
SCALINGS = (0.001, 1, 5, 20)            # mcm scalings of make_priors: the product's grid
# with fewer daily rows than assets T is rank-deficient, and under a prior of weight 0.001 N the posterior matrix is so close
# to singular that LU and Cholesky differ by up to 9 bounds (k = 2047): the reference itself is not good to the bound
SCALINGS_RANK_DEFICIENT = (0.05, 1, 5, 20)

# (k, R, layouts): N = 2 k + 24.  NSB = ceil(k / 64) pivot block rows, NS = ceil((k + R) / 64) super-tiles per side
JEFFREYS_SOLVE = (
    (510, 3, ("contiguous", "index")),  # NSB 8, NS 9: the sweep takes the unfused block steps, a run at this k the fused ones
    (512, 1, ("contiguous",)),          # the right-hand side alone in a super-tile of its own, NS 9
    (575, 16, ("contiguous", "index")),  # NSB 9, NS 10, last pivot block of 63, four full column groups
    (1023, 2, ("contiguous",)),         # NSB 16, NS 17
    (2032, 16, ("contiguous",)),        # KP 2048, NS 32: 67,584 bytes of LDS in the back substitution; k + R = 2048 exactly
    (2046, 2, ("contiguous",)),         # a column group of 2 at KP 2048
)
# (k, N, hf_days, R)
CONJUGATE_SOLVE = ((500, 250, 5, 2), (640, 400, 6, 5), (1000, 500, 22, 2))
# (k, N, hf_days, layouts)
PRIOR = (
    (500, 250, 5, ("contiguous",)),     # BASELINE configs[2]
    (511, 260, 5, ("contiguous",)),     # border column last in a super-tile, NS 8
    (512, 260, 5, ("contiguous",)),     # border column alone, NS 9 (unfused)
    (575, 300, 5, ("contiguous", "index+hf")),  # and a different intraday row count per window
    (1000, 500, 22, ("contiguous",)),   # BASELINE configs[4]: the C pass over m = 1715 rows
    (1023, 1100, 1, ("contiguous",)),   # full-rank T
    (2047, 300, 24, ("contiguous",)),   # tp_max_assets()
)


def case_id(c):
    return "-".join("+".join(x) if isinstance(x, tuple) else str(x) for x in c)


def rhs_bound(ref):
    return RHS_TOL * max(1.0, float(np.abs(ref).max()))


def aux_ratio(got, ref):
    """|got - ref| in units of atol + rtol |ref| (numpy.testing.assert_allclose passes at <= 1)."""
    return float((np.abs(got - ref) / (AUX_TOL["atol"] + AUX_TOL["rtol"] * np.abs(ref))).max())


# ---- helpers the sweep test files share -------------------------------------------------------------------------------
def make_shift(rng, W, S):
    """[W x S x 2]: shift 0 all-zero, d ~ Gamma(1, 10)/2, e ~ U(0, 50)."""
    sh = np.stack([rng.gamma(1.0, 10.0, size=(W, S)) / 2, rng.uniform(0.0, 50.0, size=(W, S))], axis=2)
    sh[:, 0, :] = 0.0
    return sh


def make_priors(rng, W, P, k, N, scalings=SCALINGS):
    """(n0 [W x P], w0 [W x P x k]): prior p is scaling scalings[(p // 2) % 4] x (ew, vw)[p % 2], n0 = N scaling U(1, 1.6), vw a
    normalised, descending log-normal vector, ew 1/k."""
    n0 = np.empty((W, P))
    w0 = np.empty((W, P, k))
    for p in range(P):
        n0[:, p] = N * scalings[(p // 2) % 4] * rng.uniform(1.0, 1.6, size=W)
        if p % 2:
            caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
            w0[:, p, :] = caps / caps.sum(axis=1, keepdims=True)
        else:
            w0[:, p, :] = 1.0 / k
    return n0, w0


def layouts(inp, seed, hf_index=False):
    """(name, panel, upload kwargs, oracle kwargs) of the contiguous layout and of one with row_idx / n_rows / col_idx /
    rf_adj over a panel with 8 more columns to choose from (n_rows within [n_r - 5, n_r], and at least k where the window
    has that many rows); `hf_index`: a third one that also has hf_row_idx and a different hf_count per window."""
    k, W, n_r, m = inp["k"], inp["W"], inp["n_r"], inp["m"]
    cont = dict(start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    yield "contiguous", inp["panel"], cont, dict(cont, n_r=n_r, m=m)
    rng = np.random.default_rng(seed)
    P = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], 8))], axis=1)
    H = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], 8))], axis=1)
    col_idx = np.stack([rng.permutation(P.shape[1])[:k] for _ in range(W)]).astype(np.int32)
    row_idx = np.stack([inp["start"][w] + np.sort(rng.choice(n_r, n_r, replace=False)) for w in range(W)]).astype(np.int32)
    n_rows = rng.integers(max(k, n_r - 5) if n_r >= k else n_r - 5, n_r + 1, size=W).astype(np.int32)
    rf_adj = rng.normal(0, 1e-4, size=(W, n_r))
    idx = dict(row_idx=row_idx, n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj, hf_panel=H, hf_start=inp["hf_start"],
               w0=inp["w0"], n0=inp["n0"])
    yield "index", P, idx, dict(idx, start=None, n_r=n_r, m=m)
    if hf_index:
        hf_row_idx = np.stack([np.sort(rng.choice(H.shape[0], m, replace=False)) for _ in range(W)]).astype(np.int32)
        hf_count = (m - 3 * np.arange(W) - 1).astype(np.int32)
        hfi = dict(idx, hf_row_idx=hf_row_idx, hf_count=hf_count)
        del hfi["hf_start"]
        yield "index+hf", P, hfi, dict(hfi, start=None, hf_start=None, n_r=n_r, m=m)


def window_X(panel, okw, k, w):
    """(X, cols) of window w, sliced the way oracle.posterior_batch slices it."""
    nr = int(okw["n_rows"][w]) if okw.get("n_rows") is not None else okw["n_r"]
    rows = (np.asarray(okw["row_idx"][w][:nr], dtype=np.int64) if okw.get("row_idx") is not None
            else np.arange(okw["start"][w], okw["start"][w] + nr))
    cols = np.asarray(okw["col_idx"][w], dtype=np.int64) if okw.get("col_idx") is not None else np.arange(k)
    X = panel[np.ix_(rows, cols)]
    if okw.get("rf_adj") is not None:
        X = X - np.asarray(okw["rf_adj"][w][:nr])[:, None]
    return X, cols


def window_Y(okw, cols, w):
    mm = int(okw["hf_count"][w]) if okw.get("hf_count") is not None else okw["m"]
    rows = (np.asarray(okw["hf_row_idx"][w][:mm], dtype=np.int64) if okw.get("hf_row_idx") is not None
            else np.arange(okw["hf_start"][w], okw["hf_start"][w] + mm))
    return okw["hf_panel"][np.ix_(rows, cols)]


def _layout(inp, seed, layout):
    for name, panel, ukw, okw in layouts(inp, seed, hf_index=layout == "index+hf"):
        if name == layout:
            return panel, ukw, okw
    raise ValueError(layout)


JEFFREYS_ONLY = ("hf_panel", "hf_start", "w0", "n0")


# ---- references of (M + d I + e 1 1') X = B ----------------------------------------------------------------------------
def shifted_solves(M, shift, B, independent):
    """x [S x R x k] = (M + d_s I + e_s 1 1')^-1 B / gamma for B [k x R], by numpy.linalg.solve (LU), and the same by
    Cholesky when `independent` (else None)."""
    k = M.shape[0]
    lu = np.empty((len(shift), B.shape[1], k))
    ch = np.empty_like(lu) if independent else None
    for s, (d, e) in enumerate(shift):
        A = M + e
        A[np.diag_indices(k)] += d
        lu[s] = np.linalg.solve(A, B).T / GAMMA
        if independent:
            ch[s] = _cholesky_solve(A, B).T / GAMMA
    return lu, ch


# ---- solve sweep, Jeffreys ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jeffreys_solve_case(k, R, layout):
    """N = 2 k + 24, W = 2, S = 3 (shift 0 all-zero), the default right-hand side plus R - 1 standard-normal columns."""
    N, seed = 2 * k + 24, 950000 + k
    inp = synthetic.make_kernel_inputs(k, N, W, seed=seed)
    rng = np.random.default_rng(seed)
    shift = make_shift(rng, W, S)
    rhs = rng.normal(size=(W, R - 1, k))
    panel, ukw, okw = _layout(inp, seed, layout)
    return dict(k=k, N=N, n_r=inp["n_r"], R=R, layout=layout, panel=panel, shift=shift, rhs=rhs, okw=okw,
                upload={key: val for key, val in ukw.items() if key not in JEFFREYS_ONLY})


@functools.lru_cache(maxsize=None)
def jeffreys_solve_reference(k, R, layout, no_center, independent=False):
    """dict(x [W, S, R, k], t [W, k], x_ind or None): M_w = T - t t'/N (the rolling window N: the default centring) or T
    (TP_FLAG_NO_CENTER) from oracle.canonical_statistics_T / _t."""
    c = jeffreys_solve_case(k, R, layout)
    x, t_all = np.empty((W, S, R, k)), np.empty((W, k))
    x_ind = np.empty_like(x) if independent else None
    for w in range(W):
        X, _ = window_X(c["panel"], c["okw"], k, w)
        T, t = oracle.canonical_statistics_T(X), oracle.canonical_statistics_t(X)
        M = T if no_center else T - np.outer(t, t) / c["N"]
        B = np.column_stack([t] + [c["rhs"][w, j] for j in range(R - 1)])
        x[w], ind = shifted_solves(M, c["shift"][w], B, independent)
        if independent:
            x_ind[w] = ind
        t_all[w] = t
    return dict(x=x, t=t_all, x_ind=x_ind)


# ---- solve sweep, conjugate --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conjugate_solve_case(k, N, hf_days, R):
    """W = 2, contiguous, no shift, the default right-hand side c S0 w0 + t plus R - 1 standard-normal columns."""
    seed = 951000 + k
    inp = synthetic.make_kernel_inputs(k, N, W, seed=seed, hf_days=hf_days)
    rhs = np.random.default_rng(seed).normal(size=(W, R - 1, k))
    panel, ukw, okw = _layout(inp, seed, "contiguous")
    return dict(k=k, N=N, n_r=inp["n_r"], m=inp["m"], R=R, panel=panel, rhs=rhs, okw=okw, upload=ukw)


@functools.lru_cache(maxsize=None)
def conjugate_solve_reference(k, N, hf_days, R, independent=False):
    """dict(x [W, 1, R, k], b0 [W, k], x_ind or None): S1 and b0 = c S0 w0 + t from oracle.conjugate_window."""
    c = conjugate_solve_case(k, N, hf_days, R)
    x, b0_all = np.empty((W, 1, R, k)), np.empty((W, k))
    x_ind = np.empty_like(x) if independent else None
    for w in range(W):
        X, cols = window_X(c["panel"], c["okw"], k, w)
        w0, n0 = c["okw"]["w0"][w], float(c["okw"]["n0"][w])
        a = oracle.conjugate_window(X, window_Y(c["okw"], cols, w), w0, n0, N, k, GAMMA, return_aux=True)[1]
        b0 = a["c"] * (a["S0"] @ w0) + a["t"]
        B = np.column_stack([b0] + [c["rhs"][w, j] for j in range(R - 1)])
        x[w], ind = shifted_solves(a["S1"], np.zeros((1, 2)), B, independent)
        if independent:
            x_ind[w] = ind
        b0_all[w] = b0
    return dict(x=x, b0=b0_all, x_ind=x_ind)


# ---- prior sweep -------------------------------------------------------------------------------------------------------
def prior_inputs(k, N, hf_days, W, P, seed):
    """(inp, n0 [W x P], w0 [W x P x k]): priors from make_priors, on SCALINGS_RANK_DEFICIENT where the daily rows are fewer
    than the assets."""
    inp = synthetic.make_kernel_inputs(k, N, W, seed=seed, hf_days=hf_days)
    scalings = SCALINGS_RANK_DEFICIENT if inp["n_r"] < k else SCALINGS
    n0, w0 = make_priors(np.random.default_rng(seed), W, P, k, N, scalings)
    return inp, n0, w0


@functools.lru_cache(maxsize=None)
def prior_case(k, N, hf_days, layout):
    """W = 2, P = 4."""
    seed = 952000 + k
    inp, n0, w0 = prior_inputs(k, N, hf_days, W, P, seed)
    panel, ukw, okw = _layout(inp, seed, layout)
    return dict(k=k, N=N, n_r=inp["n_r"], m=inp["m"], layout=layout, panel=panel, n0=n0, w0=w0, okw=okw, upload=ukw)


def prior_window_reference(c, w, independent=False):
    """(weights [P, k], aux [P, 6] = n0, n1, c, q0, q1, n1 - q1, the same two from a Cholesky solve or None) of window w of a
    prior-sweep case `c` (panel, okw, k, N, n0 [W x P], w0 [W x P x k]): oracle.conjugate_window per prior."""
    k = c["k"]
    n_prior = c["n0"].shape[1]
    X, cols = window_X(c["panel"], c["okw"], k, w)
    Y = window_Y(c["okw"], cols, w)
    wts, aux = np.empty((n_prior, k)), np.empty((n_prior, 6))
    wts_ind, aux_ind = (np.empty_like(wts), np.empty_like(aux)) if independent else (None, None)
    for p in range(n_prior):
        n0, w0 = float(c["n0"][w, p]), c["w0"][w, p]
        wts[p], a = oracle.conjugate_window(X, Y, w0, n0, c["N"], k, GAMMA, return_aux=True)
        aux[p] = (n0, a["n1"], a["c"], a["q0"], a["q1"], a["n1"] - a["q1"])
        if independent:
            w1 = _cholesky_solve(a["S1"], a["c"] * (a["S0"] @ w0) + a["t"])
            q1 = float(w1 @ (a["S1"] @ w1))
            wts_ind[p] = (a["n1"] + k + 2) * w1 / (a["n1"] - q1) / GAMMA           # ref:572-575, 836
            aux_ind[p] = (n0, a["n1"], a["c"], a["q0"], q1, a["n1"] - q1)
    return wts, aux, wts_ind, aux_ind


@functools.lru_cache(maxsize=None)
def prior_reference(k, N, hf_days, layout, independent=False):
    """dict(weights [W, P, k], aux [W, P, 6], weights_ind, aux_ind or None)."""
    c = prior_case(k, N, hf_days, layout)
    per_window = [prior_window_reference(c, w, independent) for w in range(W)]
    stack = lambda i: np.stack([r[i] for r in per_window]) if independent or i < 2 else None
    return dict(weights=stack(0), aux=stack(1), weights_ind=stack(2), aux_ind=stack(3))
