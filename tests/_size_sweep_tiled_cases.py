"""Cases, references and bounds for the tiled size sweep (tp_batch_size_sweep_tiled / Batch.size_sweep_tiled), shared by
tests/test_host_size_sweep_tiled_cases.py (CPU: are the cases well-posed?) and tests/test_gpu_size_sweep_tiled.py (GPU: do the
kernels give the oracle's numbers?).  No tests in here.

The reference is the oracle on the PREFIX columns, per (window, prior, size): oracle.conjugate_window / oracle.jeffreys_window
on the first k_s columns of the window's rows with that size's w0 - what oracle.posterior_batch computes for a batch of size
k_s.  `independent=True` solves the same prefix systems a second time by Cholesky (scipy), the conjugate nu rescale redone from
that w1: the CPU test holds the two within a tenth of the bound the GPU test applies, so a miss on the GPU is the kernel's.
Bound: atol = SOL_TOL max(1, |ref|.max()), rtol = 0; aux: AUX_TOL.  Cases and references are cached per process."""
import functools

import numpy as np

from incorporating_different_sources_amd import synthetic
from oracle import oracle

from _run_option_cases import AUX_TOL, FLAG_CENTER_BY_ROWS, FLAG_NO_CENTER, GAMMA, SOL_TOL, _cholesky_solve, sol_bound  # noqa: F401
from _tiled_sweep_cases import JEFFREYS_ONLY, SCALINGS, _layout, aux_ratio, window_X, window_Y  # noqa: F401

W = 2
P = 2
# (name, k, N, hf_days, sizes): the smallest shapes at which the geometry can go wrong.  KP = 64 ceil((k + S)/64), NS = KP/64
# super-tiles per side, NSB = ceil(k/64) pivot block rows; N = 2 k + 24
CASES = {
    "A": (144, 312, 2, (1, 16, 63, 64, 65, 128, 143, 144)),           # NSB 3, NS 3; every layout
    "B": (191, 406, 2, (100, 191)),                                   # a right-hand-side column last in a super-tile
    "C": (192, 408, 2, (64, 192)),                                    # right-hand-side column alone in a super-tile of its own
    "D": (250, 524, 3, (1, 2, 63, 64, 65, 127, 128, 129, 143, 144, 191, 192, 193, 240, 249, 250)),   # S = 16: columns straddle super-tiles 3 and 4
    "E": (520, 1064, 5, (50, 143, 256, 511, 512, 513, 519, 520)),     # NS 9: the unfused block steps
    "F": (2032, 4088, None, (1, 64, 143, 144, 500, 1000, 1023, 1024, 1025, 1500, 1984, 1985, 2000, 2030, 2031, 2032)),   # k + S = 2048, KP 2048
}
LAYOUTS_OF = {"A": ("contiguous", "index", "index+hf")}                # every other case: contiguous
CONJUGATE_CASES = ("A", "B", "C", "D", "E")
JEFFREYS_CASES = ("A", "D", "F")                                        # F: W = 1
ALL_FLAGS_CASES = ("A", "D")                                            # Jeffreys under all three centring flags
# centring flag of a Jeffreys batch -> the N oracle.jeffreys_window takes ("rows": the window's own row count)
JEFFREYS_N = {0: "N", FLAG_CENTER_BY_ROWS: "rows", FLAG_NO_CENTER: None}


def layouts_of(name):
    return LAYOUTS_OF.get(name, ("contiguous",))


def make_size_priors(rng, W, P, sizes, k, N):
    """(n0 [W x P], w0 [W x P x S x k]): even priors ew-like (1/k_s) at scaling SCALINGS[1], odd ones vw-like (a descending
    log-normal vector cut at k_s and normalised) at SCALINGS[2]; n0 = N scaling U(1, 1.6); zeros beyond k_s."""
    n0 = np.empty((W, P))
    w0 = np.zeros((W, P, len(sizes), k))
    for p in range(P):
        n0[:, p] = N * SCALINGS[1 + p % 2] * rng.uniform(1.0, 1.6, size=W)
        caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
        for s, ks in enumerate(sizes):
            w0[:, p, s, :ks] = caps[:, :ks] / caps[:, :ks].sum(axis=1, keepdims=True) if p % 2 else 1.0 / ks
    return n0, w0


@functools.lru_cache(maxsize=None)
def case(name, strategy, layout="contiguous"):
    """dict(k, N, n_r, m, sizes, W, panel, upload, okw, n0, w0): the upload kwargs of the strategy's batch, the oracle's view of
    the layout and, conjugate, the sweep's priors."""
    k, N, hf_days, sizes = CASES[name]
    conj = strategy == "conjugate"
    nw = 1 if name == "F" else W
    seed = 960000 + k
    inp = synthetic.make_kernel_inputs(k, N, nw, seed=seed, **({} if hf_days is None else dict(hf_days=hf_days)))
    panel, ukw, okw = _layout(inp, seed, layout)
    n0 = w0 = None
    if conj:
        n0, w0 = make_size_priors(np.random.default_rng(seed), nw, P, sizes, k, N)
    else:
        ukw = {key: val for key, val in ukw.items() if key not in JEFFREYS_ONLY and not key.startswith("hf_")}
    return dict(name=name, k=k, N=N, n_r=inp["n_r"], m=inp["m"] if conj else 0, sizes=list(sizes), W=nw, panel=panel, upload=ukw,
                okw=okw, n0=n0, w0=w0, inp=inp)


def conjugate_prefix_reference(X, Y, w0, n0, N, ks, independent=False):
    """(weights [k_s], aux [6] = n0, n1, c, q0, q1, n1 - q1, the same two by Cholesky or None) of one (window, prior, size)."""
    wts, a = oracle.conjugate_window(X[:, :ks], Y[:, :ks], w0[:ks], n0, N, ks, GAMMA, return_aux=True)
    aux = np.array((n0, a["n1"], a["c"], a["q0"], a["q1"], a["n1"] - a["q1"]))
    if not independent:
        return wts, aux, None, None
    w1 = _cholesky_solve(a["S1"], a["c"] * (a["S0"] @ w0[:ks]) + a["t"])
    q1 = float(w1 @ (a["S1"] @ w1))
    return wts, aux, (a["n1"] + ks + 2) * w1 / (a["n1"] - q1) / GAMMA, np.array((n0, a["n1"], a["c"], a["q0"], q1, a["n1"] - q1))


def jeffreys_prefix_reference(X, N, ks, independent=False):
    """(weights [k_s], the same by Cholesky or None); N = None: no centring."""
    wts = oracle.jeffreys_window(X[:, :ks], N, GAMMA)
    if not independent:
        return wts, None
    T, t = oracle.canonical_statistics_T(X[:, :ks]), oracle.canonical_statistics_t(X[:, :ks])
    J = T if N is None else T - np.outer(t, t) / N
    return wts, _cholesky_solve(J, t) / GAMMA


@functools.lru_cache(maxsize=None)
def conjugate_reference(name, layout="contiguous", independent=False):
    """dict(weights [W, P, S, k] zero beyond k_s, aux [W, P, S, 6], weights_ind, aux_ind or None)."""
    c = case(name, "conjugate", layout)
    k, sizes = c["k"], c["sizes"]
    wts, aux = np.zeros((c["W"], P, len(sizes), k)), np.zeros((c["W"], P, len(sizes), 6))
    wts_ind, aux_ind = (np.zeros_like(wts), np.zeros_like(aux)) if independent else (None, None)
    for w in range(c["W"]):
        X, cols = window_X(c["panel"], c["okw"], k, w)
        Y = window_Y(c["okw"], cols, w)
        for p in range(P):
            for s, ks in enumerate(sizes):
                r = conjugate_prefix_reference(X, Y, c["w0"][w, p, s], float(c["n0"][w, p]), c["N"], ks, independent)
                wts[w, p, s, :ks], aux[w, p, s] = r[0], r[1]
                if independent:
                    wts_ind[w, p, s, :ks], aux_ind[w, p, s] = r[2], r[3]
    return dict(weights=wts, aux=aux, weights_ind=wts_ind, aux_ind=aux_ind)


@functools.lru_cache(maxsize=None)
def jeffreys_reference(name, layout="contiguous", flag=0, independent=False):
    """dict(weights [W, 1, S, k] zero beyond k_s, weights_ind or None) under the centring flag `flag`."""
    c = case(name, "jeffreys", layout)
    k, sizes = c["k"], c["sizes"]
    wts = np.zeros((c["W"], 1, len(sizes), k))
    wts_ind = np.zeros_like(wts) if independent else None
    for w in range(c["W"]):
        X, _ = window_X(c["panel"], c["okw"], k, w)
        N = {"N": c["N"], "rows": X.shape[0], None: None}[JEFFREYS_N[flag]]
        for s, ks in enumerate(sizes):
            r = jeffreys_prefix_reference(X, N, ks, independent)
            wts[w, 0, s, :ks] = r[0]
            if independent:
                wts_ind[w, 0, s, :ks] = r[1]
    return dict(weights=wts, weights_ind=wts_ind)
