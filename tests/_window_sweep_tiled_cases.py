"""The case table of the tiled window sweep tests (tp_batch_window_sweep_tiled / Batch.window_sweep_tiled, k > 143):
tests/test_gpu_window_sweep_tiled.py compares the device against the oracle on it, tests/test_host_window_sweep_tiled_cases.py
checks on the CPU that the oracle alone is trustworthy on it.  No tests in here.

The table's machinery is that of tests/_window_sweep_cases.py (`rows_table`, `suffix_inputs`, `reference`, `window_rows`,
`bound`: the oracle once per length on the suffix rows): a case is (k, N) with a list of row counts for window 0; window w
uses `rows - w` where that stays valid, N_l = rows + 1 of window 0.  Inputs: synthetic.make_kernel_inputs (returns-like, so the
raw-moment centring of the tiled path's C is exact to rounding) with enough intraday days that m > k - the prior then makes S1
positive definite whatever the segment - and seed 970000 + k.

The smallest shapes at which each piece can go wrong.  NS = ceil((k + 1)/64) super-tiles per side, the border (ones) column is
column k:
  k = 144  NS 3; the first size of the call.  Every layout, every Jeffreys centring form, the L = 16 list.
  k = 191  the border column is the last column of super-tile 2
  k = 192  the border column opens a super-tile of its own (NS 4)
  k = 260  NS 5
  k = 520  NS 9: the factorisation's three-kernel form above 8 super-tiles per side.  Contiguous layout, L = 3.
Conjugate lists start at 1 row.  LIST_144 has segments of 1, 1, 2, 3, 5, 4, 11, 12, 13, 8, 24, 23, 25 and 168 rows - on, before
and after a multiple of 4 (the k-step of tw_gram_pass) and of 12 (its three-k-step software pipeline), as segment lengths and
as segment ends - and window 1 ties its first two lengths (1 and 2 - 1 rows).  Jeffreys lists start at least 16 rows above k (the
CPU test decides: the oracle must stay within a quarter of the bound)."""
import numpy as np

from incorporating_different_sources_amd import synthetic

from _size_sweep_tiled_cases import AUX_TOL, aux_ratio  # noqa: F401  (the tiled sweeps' tolerance for aux)
from _window_sweep_cases import GAMMA, JEFFREYS_FLAGS, P, TOL, W, bound, reference, rows_table, suffix_inputs, window_rows  # noqa: F401
from test_gpu_size_sweep import layouts

LIST_144 = [1, 2, 4, 7, 12, 16, 27, 39, 52, 60, 84, 107, 132, 300]
LIST16_144 = [1, 2, 3, 5, 8, 12, 13, 24, 25, 36, 37, 48, 60, 100, 200, 300]
# k: (N, conjugate row lists, Jeffreys row lists)
CASES = {
    144: (301, [LIST_144, LIST16_144], [[160, 161, 163, 166, 171, 183, 184, 300]]),
    191: (261, [[1, 2, 13, 100, 260]], [[207, 209, 236, 260]]),
    192: (261, [[1, 2, 12, 101, 260]], [[208, 211, 240, 260]]),
    260: (341, [[1, 2, 11, 130, 340]], [[276, 279, 300, 340]]),
    520: (641, [[3, 250, 640]], [[560, 600, 640]]),
}
LAYOUTS = ("contiguous", "contiguous_rf", "index")
ALL_FLAGS_K = 144                               # the three Jeffreys centring forms at this k; flag 0 elsewhere
CONTIGUOUS_ONLY = (520,)                        # one conjugate and one Jeffreys case, with a delta


def geometry(k):
    """(NS, super-tile of the border column, its column inside that super-tile)."""
    return (k + 1 + 63) // 64, k // 64, k % 64


def hf_days(k):
    return k // synthetic.BARS_PER_DAY + 1     # m = 78 hf_days - 1 > k


def problems(strategy, ks=None):
    """Every (k, list, layout, delta or not) of the table as the dict tests/_window_sweep_cases.py works on."""
    for k in (CASES if ks is None else ks):
        N, conj_lists, jeff_lists = CASES[k]
        inp = synthetic.make_kernel_inputs(k, N, W, seed=970000 + k, hf_days=hf_days(k))
        n_r = inp["n_r"]
        (_, cpanel, cukw, cokw), (_, ipanel, iukw, iokw) = list(layouts(inp, 970000 + k))
        rng = np.random.default_rng(970000 + k)
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
            for name in (("contiguous",) if k in CONTIGUOUS_ONLY else LAYOUTS):
                panel, ukw, okw = three[name]
                n_w = np.asarray(okw["n_rows"] if okw.get("n_rows") is not None else np.full(W, n_r), dtype=np.int32)
                for with_delta in ((True,) if k in CONTIGUOUS_ONLY else (False, True)):
                    yield dict(k=k, N=Nl, rows0=list(rows0), list_id=li, layout=name, strategy=strategy, inp=inp, panel=panel,
                               upload=ukw, okw=okw, n_w=n_w, rows=rows_table(rows0, n_w, 1 if strategy == "conjugate" else k + 2),
                               delta=delta if with_delta else None, n0=n0, w0=w0,
                               id=f"k{k}-list{li}-{name}-{'delta' if with_delta else 'nodelta'}")


def jeffreys_flags(k):
    return tuple(JEFFREYS_FLAGS) if k == ALL_FLAGS_K else (0,)
