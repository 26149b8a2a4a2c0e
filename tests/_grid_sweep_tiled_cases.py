"""The case table of the tiled grid sweep tests (tp_batch_grid_sweep_tiled / Batch.grid_sweep_tiled, k > 143):
tests/test_gpu_grid_sweep_tiled.py compares the device against the oracle on it, tests/test_host_grid_sweep_tiled_cases.py checks
on the CPU that the oracle alone is trustworthy on it.  No tests in here.

A case is a problem of the tiled window sweep's table (tests/_window_sweep_tiled_cases.py: k, N, a list of row counts, W = 2
windows, P = 2 priors, three layouts, delta = None and delta ~ N(0, 1e-6)) with a list of sizes on top.  w0 [W x P x S x k] is
that problem's vector cut at k_s and normalised, zeros beyond k_s (`_grid_sweep_cases._with_sizes`).  The reference is
oracle.posterior_batch once per (prior, length, size) on the suffix rows and the prefix columns (`_grid_sweep_cases.reference`),
computed once per problem and shared.

The smallest shapes at which each piece can go wrong.  KP = 64 ceil((k + S)/64), NS = KP/64 super-tiles per side, the
right-hand-side columns are k .. k + S - 1:
  k = 144  [1, 63, 64, 65, 128, 143, 144]  NS 3; prefixes on, before and after a 64-row block.  Every layout, the three Jeffreys
                                           centring forms; conjugate: LIST_144 cut to its first 6 and last 2 lengths.
  k = 144  SIZES16_144 (S = 16)            the four size groups of the solve, with LIST16_144 (L = 16).  P = 1, index layout with
                                           a delta, once.
  k = 191  [100, 191] and [191]            S = 1: column 191 is the arena's last column (KP 192).  S = 2: the right-hand sides
                                           straddle super-tiles 2 and 3 (NS 4).
  k = 192  [64, 129, 192]                  the right-hand-side columns open a super-tile of their own
  k = 260  [1, 144, 200, 256, 257, 260]    NS 5; sizes below 144 ride along in a tiled entry
  k = 520  [100, 300, 520]                 NS 9: the unfused block steps.  Contiguous layout, L = 3, with a delta.
The Jeffreys lists are the window table's own: rows >= k + 16 at the LARGEST size, so every prefix has more to spare."""
import functools

import numpy as np

import _window_sweep_tiled_cases as wcases
from _grid_sweep_cases import _with_sizes, prefix_inputs, reference  # noqa: F401  (the reference: the oracle per (prior, length, size))
from _window_sweep_tiled_cases import AUX_TOL, GAMMA, JEFFREYS_FLAGS, LIST16_144, LIST_144, TOL, W, aux_ratio, bound, hf_days, window_rows  # noqa: F401

P = wcases.P
# k: the size lists of the k's first list of lengths
SIZES = {144: [[1, 63, 64, 65, 128, 143, 144]], 191: [[100, 191], [191]], 192: [[64, 129, 192]],
         260: [[1, 144, 200, 256, 257, 260]], 520: [[100, 300, 520]]}
SIZES16_144 = [1, 2, 31, 63, 64, 65, 96, 100, 127, 128, 129, 140, 141, 142, 143, 144]
CUT_144 = list(range(6)) + [len(LIST_144) - 2, len(LIST_144) - 1]      # conjugate, k = 144: the first 6 and the last 2 lengths of LIST_144


def geometry(k, S):
    """(KP, NS, NSB, super-tiles the right-hand-side columns k .. k + S - 1 lie in)."""
    KP = 64 * ((k + S + 63) // 64)
    return KP, KP // 64, (k + 63) // 64, sorted({(k + s) // 64 for s in range(S)})


def cut_lengths(pr, ls, tag=""):
    """The problem with the lengths `ls` of its list alone."""
    ls = list(ls)
    return dict(pr, N=np.ascontiguousarray(pr["N"][ls]), rows0=[pr["rows0"][l] for l in ls], rows=np.ascontiguousarray(pr["rows"][:, ls]),
                delta=None if pr["delta"] is None else np.ascontiguousarray(pr["delta"][:, ls]),
                n0=np.ascontiguousarray(pr["n0"][:, :, ls]), id=pr["id"] + tag)


@functools.lru_cache(maxsize=None)
def _problems(strategy):
    out = []
    for pr in wcases.problems(strategy):
        k = pr["k"]
        if pr["list_id"] == 0:
            if strategy == "conjugate" and k == 144:
                pr = cut_lengths(pr, CUT_144)
            for sizes in SIZES[k]:
                out.append(_with_sizes(pr, sizes, P, f"-S{len(sizes)}"))
        elif strategy == "conjugate" and pr["layout"] == "index" and pr["delta"] is not None:
            assert pr["rows0"] == LIST16_144
            out.append(_with_sizes(pr, SIZES16_144, 1, "-S16"))
    return tuple(out)


def problems(strategy, ks=None):
    """The table as dicts: the tiled window sweep's problem plus `sizes` [S], `P`, `n0` [W x P x L] and `w0g` [W x P x S x k]."""
    return [pr for pr in _problems(strategy) if ks is None or pr["k"] in ks]


def jeffreys_flags(k):
    return wcases.jeffreys_flags(k)
