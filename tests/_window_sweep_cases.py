"""The case table of the window sweep tests (tests/test_gpu_window_sweep.py compares the device against the oracle on it,
tests/test_host_window_sweep_cases.py checks on the CPU that the oracle alone is trustworthy on it).

A case is (k, N) with a list of row counts for window 0; window w uses `rows - w` where that stays valid (>= 1, Jeffreys:
>= k + 2, so that the scatter centred by the row count keeps a rank above k; otherwise the count stays, which ties it with its
neighbour) and never more than the window's own rows, so the windows differ.  N_l = rows + 1
of window 0.  Inputs: synthetic.make_kernel_inputs(k, N, 2, seed=920000 + k); three layouts - contiguous, contiguous with a
per-row risk-free adjustment rf_adj ~ N(0, 1e-4), and the index layout of the size-sweep tests' `layouts` helper -, each with
delta = None and with delta ~ N(0, 1e-6).

What the lists cover: NT = 1, 3 and 9 tiles per side; segments of 1, 2, 3 and 5 rows; segment ends on, before and after a
multiple of 4 (the k-step) and of 64 (the staging loads); a tie; L = 16.  Jeffreys at k = 143 starts at 160 rows: at 144 the
oracle itself uses 0.16 of the bound."""
import numpy as np

from incorporating_different_sources_amd import synthetic
from oracle import oracle
from test_gpu_size_sweep import layouts

GAMMA = 5.0
TOL = 1e-10                                    # weights: atol = TOL max(1, |ref|.max()), rtol = 0 (tests/test_gpu_size_sweep.py)
AUX_RTOL, AUX_ATOL = 1e-11, 1e-14              # aux[..., :6]
W, P = 2, 2

LIST16_143 = [144, 145, 147, 150, 155, 160, 176, 192, 200, 255, 256, 257, 300, 320, 398, 399]
# k: (N, conjugate row lists, Jeffreys row lists)
CASES = {
    5: (40, [[1, 3, 4, 5, 8, 13, 39]], [[7, 8, 9, 13, 39]]),
    33: (130, [[1, 2, 4, 5, 63, 64, 65, 129]], [[48, 63, 64, 65, 66, 100, 129]]),
    143: (400, [[144, 160, 200, 255, 256, 257, 300, 399], LIST16_143], [[160, 200, 255, 256, 257, 300, 399]]),
}
LAYOUTS = ("contiguous", "contiguous_rf", "index")
JEFFREYS_FLAGS = {0: {}, 1: dict(center_rows=True), 2: dict(no_center=True)}      # TP_FLAG_* -> oracle keywords


def rows_table(rows0, n_w, least=1):
    """[W x L]: window w uses rows0 - w where that is >= `least`, at most its own n_w rows."""
    out = np.empty((len(n_w), len(rows0)), dtype=np.int32)
    for w, nw in enumerate(n_w):
        out[w] = [min(r - w if r - w >= least else r, int(nw)) for r in rows0]
    assert (out >= 1).all() and (np.diff(out, axis=1) >= 0).all()
    return out


def problems(strategy, ks=None):
    """Every (k, list, layout, delta or not) of the table as a dict: `panel`, `upload` (keywords of Batch.upload), `okw`
    (keywords of oracle.posterior_batch), `N` [L], `rows` [W x L], `delta` [W x L x n_r] or None, `n0` [W x P x L] and `w0`
    [W x P x k] (conjugate), `n_w` [W], `inp`."""
    for k in (CASES if ks is None else ks):
        N, conj_lists, jeff_lists = CASES[k]
        inp = synthetic.make_kernel_inputs(k, N, W, seed=920000 + k)
        n_r = inp["n_r"]
        lay = list(layouts(inp, 920000 + k))
        (_, cpanel, cukw, cokw), (_, ipanel, iukw, iokw) = lay
        rng = np.random.default_rng(920000 + k)
        rf = rng.normal(0.0, 1e-4, size=(W, n_r))
        three = {"contiguous": (cpanel, cukw, cokw),
                 "contiguous_rf": (cpanel, dict(cukw, rf_adj=rf), dict(cokw, rf_adj=rf)),
                 "index": (ipanel, iukw, iokw)}
        for li, rows0 in enumerate(conj_lists if strategy == "conjugate" else jeff_lists):
            L = len(rows0)
            Nl = np.asarray(rows0, dtype=np.int32) + 1
            n0 = np.empty((W, P, L))
            for p in range(P):
                n0[:, p, :] = Nl[None, :] * (1, 5)[p % 2] * rng.uniform(1.0, 1.6, size=(W, L))
            caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
            w0 = np.stack([np.full((W, k), 1.0 / k), caps / caps.sum(axis=1, keepdims=True)], axis=1)
            delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))
            for name in LAYOUTS:
                panel, ukw, okw = three[name]
                n_w = np.asarray(okw["n_rows"] if okw.get("n_rows") is not None else np.full(W, n_r), dtype=np.int32)
                for with_delta in (False, True):
                    yield dict(k=k, N=Nl, rows0=list(rows0), list_id=li, layout=name, strategy=strategy, inp=inp, panel=panel,
                               upload=ukw, okw=okw, n_w=n_w, rows=rows_table(rows0, n_w, 1 if strategy == "conjugate" else k + 2),
                               delta=delta if with_delta else None, n0=n0, w0=w0,
                               id=f"k{k}-list{li}-{name}-{'delta' if with_delta else 'nodelta'}")


def suffix_inputs(pr, l):
    """Keywords of oracle.posterior_batch for length l: row_idx = the suffix, n_rows = rows[:, l], rf_adj + delta_l aligned to
    the suffix, the window's own columns."""
    okw, rows, n_r = pr["okw"], pr["rows"], pr["inp"]["n_r"]
    row_idx = np.zeros((W, n_r), dtype=np.int64)
    adj = np.zeros((W, n_r))
    for w in range(W):
        nw, r = int(pr["n_w"][w]), int(rows[w, l])
        full = (np.asarray(okw["row_idx"][w][:nw], dtype=np.int64) if okw.get("row_idx") is not None
                else np.arange(okw["start"][w], okw["start"][w] + nw))
        row_idx[w, :r] = full[nw - r:]
        a = np.zeros(nw) if okw.get("rf_adj") is None else np.asarray(okw["rf_adj"][w][:nw], dtype=np.float64).copy()
        if pr["delta"] is not None:
            a = a + pr["delta"][w, l, :nw]
        adj[w, :r] = a[nw - r:]
    kw = {key: val for key, val in okw.items() if key not in ("w0", "n0", "start", "row_idx", "n_rows", "rf_adj")}
    if pr["strategy"] == "jeffreys":
        kw = {key: val for key, val in kw.items() if not key.startswith("hf_") and key != "m"}
    return dict(kw, start=None, row_idx=row_idx, n_rows=rows[:, l].copy(), rf_adj=adj)


def reference(pr, flag=0):
    """oracle.posterior_batch once per (prior, length) -> (weights [W, P', L, k], status, aux [W, P', L, 8]); P' = 1 for Jeffreys."""
    k, L = pr["k"], len(pr["N"])
    conj = pr["strategy"] == "conjugate"
    Pn = P if conj else 1
    ref = np.zeros((W, Pn, L, k))
    rstat = np.zeros((W, Pn, L), dtype=np.int32)
    raux = np.zeros((W, Pn, L, 8))
    for l in range(L):
        kw = suffix_inputs(pr, l)
        for p in range(Pn):
            pri = dict(w0=np.ascontiguousarray(pr["w0"][:, p]), n0=np.ascontiguousarray(pr["n0"][:, p, l])) if conj else JEFFREYS_FLAGS[flag]
            ref[:, p, l], rstat[:, p, l], raux[:, p, l] = oracle.posterior_batch(pr["strategy"], k, int(pr["N"][l]), GAMMA, pr["panel"],
                                                                                 **kw, **pri)
    return ref, rstat, raux


def window_rows(pr, w, l):
    """(X, Y): the daily rows of length l of window w as the definition reads them - the suffix, minus rf_adj, minus delta - and
    the window's intraday rows (None for Jeffreys), formed here from the layout, not by the oracle's driver."""
    kw = suffix_inputs(pr, l)
    r = int(pr["rows"][w, l])
    cols = np.asarray(kw["col_idx"][w], dtype=np.int64)
    X = pr["panel"][np.ix_(kw["row_idx"][w, :r], cols)] - kw["rf_adj"][w, :r, None]
    if pr["strategy"] != "conjugate":
        return X, None
    mm = int(kw["hf_count"][w]) if kw.get("hf_count") is not None else kw["m"]
    hrows = (np.asarray(kw["hf_row_idx"][w][:mm], dtype=np.int64) if kw.get("hf_row_idx") is not None
             else np.arange(kw["hf_start"][w], kw["hf_start"][w] + mm))
    return X, kw["hf_panel"][np.ix_(hrows, cols)]


def bound(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))
