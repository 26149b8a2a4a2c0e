"""Cases, references and bounds for batches that run "with options" (tp_batch_set_rhs / keep_rhs / set_shift, the centring
flags, tp_batch_download_matrix), shared by tests/test_host_run_option_cases.py (CPU: are the cases well-posed?) and
tests/test_gpu_run_options.py (GPU: do the kernels give the oracle's numbers?).  No tests in here.

Every reference is built from oracle.oracle.  The `independent_*` functions solve the same systems a second time by Cholesky
(scipy) on the matrix assembled from the oracle's own T, t, S0: the CPU test holds the two within a tenth of the bound the GPU
test applies, so a miss on the GPU is the kernel's, not the reference's."""
import numpy as np

from incorporating_different_sources_amd import synthetic
from oracle import oracle

GAMMA = 5.0
FLAG_CENTER_BY_ROWS, FLAG_NO_CENTER = 1, 2           # TP_FLAG_* of include/tangency_posterior.h
FLAGS = (0, FLAG_CENTER_BY_ROWS, FLAG_NO_CENTER)
LAYOUTS = ("contiguous", "index")
TILE_COUNTS = tuple(range(1, 16))                    # NT = ceil((k + 1) / 16) of the register-tile kernel, k <= 239
TILED_SIZES = (240, 255, 256, 257, 320)              # border column inside / last in / alone in a 64-wide super-tile; 5 block rows
PORTFOLIO_SIZES = (150, 239, 256)

# the bounds the project already holds these quantities to
SOL_TOL = 1e-10      # solutions and weights: atol = SOL_TOL max(1, |ref|.max()), rtol = 0   (test_gpu_parity, test_gpu_solve_sweep)
RHS_TOL = 1e-12      # kept right-hand side: |got - ref|.max() <= RHS_TOL max(1, |ref|.max())   (test_gpu_solve_sweep)
MATRIX_TOL = dict(rtol=1e-11, atol=1e-17)            # read-back matrices (test_helper_functions_match_reference)
AUX_TOL = dict(rtol=1e-11, atol=1e-14)               # conjugate aux [:6]
# default against row-count centring on ragged windows: the references must be this far apart (1e4 bounds) or the case
# could not tell an ignored flag from an honoured one; on the CPU they are 0.025 .. 0.2 apart
DISCRIMINATE = 1e4 * SOL_TOL


def small_matrix_blas():
    """A context in which BLAS runs on one thread, where threadpoolctl is installed (speed only: at k <= 320 numpy's and
    scipy's thread pools spend more time waiting for each other than solving); otherwise a context that does nothing."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


def sizes_of_tile_count(nt):
    """Every k the register-tile kernel serves with NT = nt tiles per side."""
    return [k for k in range(16 * nt - 16, 16 * nt) if k >= 1]


def border_sizes_of_tile_count(nt):
    """The border column alone in the last tile, next to that, and k + 1 = 0 mod 16."""
    return [k for k in (16 * nt - 16, 16 * nt - 15, 16 * nt - 1) if k >= 1]


def sol_bound(ref):
    return SOL_TOL * max(1.0, float(np.abs(ref).max()))


# ---- cases -------------------------------------------------------------------------------------------------------------
def make_case(strategy, k, layout, W, seed=None):
    """One batch: Jeffreys with N = 2 k + 24 rows (well-posed at every size and option set), conjugate with hf_days = 1 and
    N = max(k + 30, 40) as in the every-size test of the wave kernel.  `layout` "contiguous": rolling windows by `start`;
    "index": a panel 8 columns wider with a random k-subset per window, sorted row lists, ragged n_rows in [n_r - 7, n_r] with
    at least one window below n_r, rf_adj ~ N(1e-4, 3e-5) per row and, conjugate, intraday row lists with hf_count >= m - 25.
    Returns a dict: k, N, n_r, m, W, panel, `upload` (keywords of Batch.upload besides the panel), `oracle` (keywords of
    oracle.posterior_batch besides strategy, k, N, gamma, panel), and the option values of the runs: shift [W x 2] (window 0
    unshifted, d ~ Gamma(1, 10)/2, e ~ U(0, 50)) and rhs [W x k], standard normal for Jeffreys and N(0, 0.05^2) for the
    conjugate strategy: there w1 = S1^-1 rhs goes through the nu rescale, and at the scale of the default right-hand side
    (|t| ~ 0.1) w1'S1 w1 stays well below n1, so the denominator is positive and the status TP_STATUS_OK."""
    conj = strategy == "conjugate"
    N = max(k + 30, 40) if conj else 2 * k + 24
    seed = (930000 if conj else 920000) + k if seed is None else seed
    inp = synthetic.make_kernel_inputs(k, N, W, seed=seed, hf_days=1)
    n_r, m = inp["n_r"], inp["m"]
    rng = np.random.default_rng(seed + (500 if layout == "index" else 0))
    shift = np.column_stack([rng.gamma(1.0, 10.0, W) / 2, rng.uniform(0.0, 50.0, W)])
    shift[0] = 0.0
    case = dict(strategy=strategy, k=k, N=N, n_r=n_r, m=m, W=W, layout=layout, shift=shift,
                rhs=rng.normal(size=(W, k)) * (0.05 if conj else 1.0),
                w0=inp["w0"], n0=inp["n0"])
    prior = dict(w0=inp["w0"], n0=inp["n0"]) if conj else {}
    if layout == "contiguous":
        up = dict(start=inp["start"], **prior)
        if conj:
            up.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"])
        case.update(panel=inp["panel"], upload=up, oracle=dict(up, n_r=n_r, **(dict(m=m) if conj else {})))
        return case
    assert layout == "index"
    P = np.concatenate([inp["panel"], rng.normal(3e-4, 0.014, size=(inp["panel"].shape[0], 8))], axis=1)
    col_idx = np.stack([rng.permutation(P.shape[1])[:k] for _ in range(W)]).astype(np.int32)
    row_idx = np.stack([np.sort(rng.choice(P.shape[0], n_r, replace=False)) for _ in range(W)]).astype(np.int32)
    n_rows = rng.integers(n_r - 7, n_r + 1, size=W).astype(np.int32)
    n_rows[rng.integers(W)] = n_r - 1 - rng.integers(6)                     # at least one window below n_r
    rf_adj = rng.normal(1e-4, 3e-5, size=(W, n_r))
    up = dict(row_idx=row_idx, n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj, **prior)
    if conj:
        H = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], 8))], axis=1)
        hf_row_idx = np.stack([np.sort(rng.choice(H.shape[0], m, replace=False)) for _ in range(W)]).astype(np.int32)
        hf_count = rng.integers(m - 25, m + 1, size=W).astype(np.int32)
        up.update(hf_panel=H, hf_row_idx=hf_row_idx, hf_count=hf_count)
    case.update(panel=P, upload=up, oracle=dict(up, start=None, n_r=n_r, **(dict(m=m, hf_start=None) if conj else {})))
    return case


def window_X(case, w):
    """The excess returns of window w, sliced the way oracle.posterior_batch slices them."""
    o = case["oracle"]
    nr = int(o["n_rows"][w]) if o.get("n_rows") is not None else case["n_r"]
    rows = (np.asarray(o["row_idx"][w][:nr], dtype=np.int64) if o.get("row_idx") is not None
            else np.arange(o["start"][w], o["start"][w] + nr))
    cols = np.asarray(o["col_idx"][w], dtype=np.int64) if o.get("col_idx") is not None else np.arange(case["k"])
    X = case["panel"][np.ix_(rows, cols)]
    if o.get("rf_adj") is not None:
        X = X - np.asarray(o["rf_adj"][w][:nr])[:, None]
    return X


def window_Y(case, w):
    o = case["oracle"]
    mm = int(o["hf_count"][w]) if o.get("hf_count") is not None else case["m"]
    rows = (np.asarray(o["hf_row_idx"][w][:mm], dtype=np.int64) if o.get("hf_row_idx") is not None
            else np.arange(o["hf_start"][w], o["hf_start"][w] + mm))
    cols = np.asarray(o["col_idx"][w], dtype=np.int64) if o.get("col_idx") is not None else np.arange(case["k"])
    return o["hf_panel"][np.ix_(rows, cols)]


# ---- Jeffreys ----------------------------------------------------------------------------------------------------------
# the runs of one uploaded batch, in the order the GPU test makes them: (name, shifted?, caller's right-hand side?)
JEFFREYS_RUNS = (("plain", False, False), ("shift", True, False), ("shift+rhs", True, True))


def jeffreys_reference(case, flag, shifted, with_rhs):
    """oracle.posterior_batch: weights [W x k] = (J + d I + e 1 1')^-1 (t or rhs) / gamma with the flag's centring."""
    wts, status, _ = oracle.posterior_batch(
        "jeffreys", case["k"], case["N"], GAMMA, case["panel"], rhs=case["rhs"] if with_rhs else None,
        shift=case["shift"] if shifted else None, center_rows=flag == FLAG_CENTER_BY_ROWS, no_center=flag == FLAG_NO_CENTER,
        **case["oracle"])
    assert (status == 0).all()
    return wts


def jeffreys_t(case):
    """t = X'1 of every window: what a default run solves for and keep_rhs keeps."""
    return np.stack([oracle.canonical_statistics_t(window_X(case, w)) for w in range(case["W"])])


def _cholesky_solve(M, b):
    from scipy.linalg import cho_factor, cho_solve
    return cho_solve(cho_factor(M), b)


def independent_jeffreys(case, flag, shifted, with_rhs):
    """The same solutions by Cholesky on the matrix assembled from the oracle's own T and t."""
    k = case["k"]
    out = np.empty((case["W"], k))
    for w in range(case["W"]):
        X = window_X(case, w)
        T, t = oracle.canonical_statistics_T(X), oracle.canonical_statistics_t(X)
        M = T.copy()
        if flag != FLAG_NO_CENTER:
            M -= np.outer(t, t) / (X.shape[0] if flag == FLAG_CENTER_BY_ROWS else case["N"])
        if shifted:
            M += case["shift"][w, 0] * np.eye(k) + case["shift"][w, 1] * np.ones((k, k))
        out[w] = _cholesky_solve(M, case["rhs"][w] if with_rhs else t) / GAMMA
    return out


# ---- conjugate ---------------------------------------------------------------------------------------------------------
def _rescaled(a, w1, k):
    """ref:572-575, 836 from w1: (weights, q1, denom)."""
    q1 = float(w1 @ (a["S1"] @ w1))
    denom = a["n1"] - q1
    return (a["n1"] + k + 2) * w1 / denom / GAMMA, q1, denom


def conjugate_reference(case, solve=None):
    """Per batch, from oracle.conjugate_window(..., return_aux=True): weights [W x k], aux [W x 6] = n0, n1, c, q0, q1, denom,
    b0 [W x k] = c S0 w0 + t (the kept right-hand side), the same three with the caller's right-hand side r in place of b0 -
    w1 = solve(S1, r), weights = (n1 + k + 2) w1 / (n1 - w1'S1 w1) / gamma, aux slots 4 and 5 from that w1 - and the window
    dicts (T, t, S0, S1, c, ...) themselves.  `solve`: the solver of the caller's systems AND, when given, of the default one
    (the independent Cholesky path of the CPU test); default: the oracle's own w1 and numpy.linalg.solve."""
    k, W = case["k"], case["W"]
    out = dict(weights=np.empty((W, k)), aux=np.empty((W, 6)), b0=np.empty((W, k)), weights_rhs=np.empty((W, k)),
               aux_rhs=np.empty((W, 6)), windows=[])
    for w in range(W):
        n0 = float(case["n0"][w])
        wts, a = oracle.conjugate_window(window_X(case, w), window_Y(case, w), case["w0"][w], n0, case["N"], k, GAMMA,
                                         return_aux=True)
        b0 = a["c"] * (a["S0"] @ case["w0"][w]) + a["t"]
        if solve is None:
            out["weights"][w], q1, denom = wts, a["q1"], a["n1"] - a["q1"]
        else:
            out["weights"][w], q1, denom = _rescaled(a, solve(a["S1"], b0), k)
        out["aux"][w] = (n0, a["n1"], a["c"], a["q0"], q1, denom)
        out["b0"][w] = b0
        out["weights_rhs"][w], q1, denom = _rescaled(a, (solve or np.linalg.solve)(a["S1"], case["rhs"][w]), k)
        out["aux_rhs"][w] = (n0, a["n1"], a["c"], a["q0"], q1, denom)
        out["windows"].append(a)
    return out


def independent_conjugate(case):
    return conjugate_reference(case, solve=_cholesky_solve)


# ---- portfolios above the solve sweep's largest universe -------------------------------------------------------------
def portfolio_case(k, dates=3):
    """A `batch.pack_windows`-shaped `kw` in the index layout (start None, row_idx, n_rows, col_idx, rf_adj) with N = 2 k + 24,
    and 8 fixed Greyserman draws xi ~ U(-1000, 1000), eta ~ Gamma(1, 10).  Returns (case, kw, (xi, eta))."""
    case = make_case("jeffreys", k, "index", dates, seed=940000 + k)
    kw = dict(panel=case["panel"], start=None, n_r=case["n_r"], **case["upload"])
    rng = np.random.default_rng(940000 + k)
    return case, kw, (rng.uniform(-1000.0, 1000.0, 8), rng.gamma(1.0, 10.0, 8))


def jorion_reference(case):
    return np.stack([oracle.jorion_window(window_X(case, w), GAMMA) for w in range(case["W"])])


def jorion_from(case, solve):
    """portfolio_calculations._jorion_from_solves on host solves with the row-count-centred scatter."""
    from incorporating_different_sources_amd import portfolio_calculations as pc
    k, W = case["k"], case["W"]
    x_t, x_one, ts, n = np.empty((W, k)), np.empty((W, k)), np.empty((W, k)), np.empty(W)
    for w in range(W):
        X = window_X(case, w)
        T, t = oracle.canonical_statistics_T(X), oracle.canonical_statistics_t(X)
        J = T - np.outer(t, t) / X.shape[0]
        x_t[w], x_one[w], ts[w], n[w] = solve(J, t), solve(J, np.ones(k)), t, X.shape[0]
    return pc._jorion_from_solves(x_t, x_one, ts, n, k, GAMMA)


def greyserman_from(case, draws, solve=np.linalg.solve):
    """portfolio_calculations._greyserman_from_solves on host solves of (T + eta_b/2 I) u = t and = 1: the device-free
    stand-in of test_greyserman_host_algebra_beats_the_references_own_noise (oracle.greyserman_window inverts D_h by LU and
    is only good to ~1e-6)."""
    from incorporating_different_sources_amd import portfolio_calculations as pc
    k, W = case["k"], case["W"]
    xi, eta = draws
    out = np.empty((W, k))
    for w in range(W):
        X = window_X(case, w)
        T, t = oracle.canonical_statistics_T(X), oracle.canonical_statistics_t(X)
        u_t = np.array([solve(T + e / 2 * np.eye(k), t) for e in eta])
        u_1 = np.array([solve(T + e / 2 * np.eye(k), np.ones(k)) for e in eta])
        out[w] = pc._greyserman_from_solves(u_t[None], u_1[None], t[None], [X.shape[0]], xi[None], eta[None], k, GAMMA)[0]
    return out
