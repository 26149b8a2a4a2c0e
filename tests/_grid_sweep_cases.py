"""The case table of the grid sweep tests (tests/test_gpu_grid_sweep.py compares the device against the oracle on it,
tests/test_host_grid_sweep_cases.py checks on the CPU that the oracle alone is trustworthy on it).

A case is a problem of the window sweep's table (tests/_window_sweep_cases.py: k, N, a list of row counts, W = 2 windows, three
layouts, delta = None and delta ~ N(0, 1e-6)) with a list of sizes on top:

    k = 5   (NT 1)   sizes [1, 2, 5]                 the k = 5 lists
    k = 33  (NT 3)   sizes [1, 16, 17, 32, 33]       the k = 33 lists
    k = 143 (NT 9)   sizes [8, 64, 65, 128, 143]     the first k = 143 list
    k = 143, once    SIZES16_143 (S = 16)            LIST16_143 (L = 16), P = 1, index layout with a delta

The sizes sit on, before and after the 32-lane boundary of the fill's row groups and the 64-lane boundary of the back
substitution.  The Jeffreys lists keep rows >= k + 2 at the LARGEST size, so every smaller universe has rows to spare.  Priors:
n0 [W x P x L] of the window sweep's problem; w0 [W x P x S x k] is that problem's vector cut at k_s and normalised (p = 0: equal
weights, p = 1: a descending log-normal vector), zeros beyond k_s.

The reference is oracle.posterior_batch once per (prior, length, size) on the suffix rows (`_window_sweep_cases.suffix_inputs`)
and the first k_s columns, computed once per problem and shared."""
import functools

import numpy as np

from oracle import oracle

import _window_sweep_cases as wcases
from _window_sweep_cases import GAMMA, TOL, AUX_RTOL, AUX_ATOL, W, JEFFREYS_FLAGS, bound, window_rows      # noqa: F401

SIZES = {5: [1, 2, 5], 33: [1, 16, 17, 32, 33], 143: [8, 64, 65, 128, 143]}
SIZES16_143 = [1, 2, 9, 31, 32, 33, 63, 64, 65, 96, 100, 127, 128, 129, 142, 143]


def _with_sizes(pr, sizes, P, tag=""):
    k = pr["k"]
    w0 = np.zeros((W, P, len(sizes), k))
    for s, ks in enumerate(sizes):
        cut = pr["w0"][:, :P, :ks]
        w0[:, :, s, :ks] = cut / cut.sum(axis=-1, keepdims=True)
    return dict(pr, sizes=list(sizes), P=P, n0=np.ascontiguousarray(pr["n0"][:, :P]), w0g=w0, id=pr["id"] + tag)


@functools.lru_cache(maxsize=None)
def _problems(strategy):
    out = []
    for pr in wcases.problems(strategy):
        if pr["list_id"] == 0:
            out.append(_with_sizes(pr, SIZES[pr["k"]], wcases.P))
        elif strategy == "conjugate" and pr["layout"] == "index" and pr["delta"] is not None:
            assert pr["rows0"] == wcases.LIST16_143
            out.append(_with_sizes(pr, SIZES16_143, 1, "-S16"))
    return tuple(out)


def problems(strategy, ks=None):
    """The table as dicts: the window sweep's problem plus `sizes` [S], `P`, `n0` [W x P x L] and `w0g` [W x P x S x k]."""
    return [pr for pr in _problems(strategy) if ks is None or pr["k"] in ks]


def prefix_inputs(pr, l, ks):
    """Keywords of oracle.posterior_batch for (length l, size ks): the suffix rows, the first ks of the window's own columns."""
    kw = wcases.suffix_inputs(pr, l)
    return dict(kw, col_idx=np.ascontiguousarray(np.asarray(kw["col_idx"])[:, :ks]))


_REF = {}


def reference(pr, flag=0):
    """oracle.posterior_batch once per (prior, length, size) -> (weights [W, P', L, S, k] zero beyond k_s, status [W, P', L, S],
    aux [W, P', L, S, 8]); P' = 1 for Jeffreys.  Computed once per (problem, flag); do not write into it."""
    key = (pr["strategy"], pr["id"], flag)
    if key in _REF:
        return _REF[key]
    k, L, sizes = pr["k"], len(pr["N"]), pr["sizes"]
    conj = pr["strategy"] == "conjugate"
    Pn = pr["P"] if conj else 1
    ref = np.zeros((W, Pn, L, len(sizes), k))
    rstat = np.zeros((W, Pn, L, len(sizes)), dtype=np.int32)
    raux = np.zeros((W, Pn, L, len(sizes), 8))
    for l in range(L):
        for s, ks in enumerate(sizes):
            kw = prefix_inputs(pr, l, ks)
            for p in range(Pn):
                pri = (dict(w0=np.ascontiguousarray(pr["w0g"][:, p, s, :ks]), n0=np.ascontiguousarray(pr["n0"][:, p, l])) if conj
                       else JEFFREYS_FLAGS[flag])
                wts, st, aux = oracle.posterior_batch(pr["strategy"], ks, int(pr["N"][l]), GAMMA, pr["panel"], **kw, **pri)
                ref[:, p, l, s, :ks], rstat[:, p, l, s], raux[:, p, l, s] = wts, st, aux[:, :8]
    for a in (ref, rstat, raux):
        a.setflags(write=False)
    _REF[key] = (ref, rstat, raux)
    return _REF[key]
