"""The device-fed backtest replay above k = 512 and behind the tiled sweeps (-m gpu): `replay_kernel<SPL, true>` in the forms
tests/test_gpu_replay_batch.py does not reach - the classes of 8, 16 and 32 slots per lane at their edges, the late form (16
and 32 slots: the row of a rebalancing date is resolved and loaded after the mark to market) with patches, with flagged source
rows, behind a sweep's layout, next to other classes in one call and under the summary - and `tp_replay_run_batch` reading the
workspaces the tiled sweeps write.

Yardsticks, never the code under test.  (1) Byte for byte against the merged path, as in tests/test_gpu_replay_batch.py:
download the source, scale and patch in numpy with the host's `1.0 / g * w`, `Device.replay` on the dense rows
(tests/test_gpu_replay_large.py pins that kernel to the long-double truth in every class).  (2) The long-double truth of
tests/_replay_reference.py at RTOL = 1e-10, ATOL = 1e-12, whose derivation (tests/_replay_cases.py) asks for rows of gross
exposure 2, returns as `_common` draws them and at most 23 days between rebalancing dates: test C asserts the three.

Sources: Jeffreys batches of random normal rows, n_r = k + max(24, k / 8), one per k and shared by the tests (window 4 of each
holds one NaN: its status is not OK, the others' are); W = R = 4 .. 6; D = reb_day[-1] + 3.

    test                                        SPL        source                        patches            flagged
    A run_source_at_the_class_edges             8 16 32    run                           -                  -
    B patches_in_the_late_form                  16 32      run                           0, last, 2 adjacent,  -
                                                                                          all, none; ld k, k+3
    C every_row_a_patch_against_the_truth       16 32      run (the flagged window)      every date         under the patches
    D a_flagged_row_... (middle)                16 32      run                           the twin's         date 4 of 6
    D a_flagged_row_... (first / last date)     1 32       run                           the twin's         date 0; date 3 of 4
    E every_tiled_source_constant_...           4 (2)      prior, size, window, grid     -                  -
                                                           tiled, conjugate k = 144
    E tiled_grid_sweep_two_classes              2 + 16     grid tiled, k = 520           -                  -
    E tiled_size_sweep_four_classes             1 8 16 32  size tiled, k = 1100          every class; ld 1100, 40   -
    E the_tiled_size_sweeps_own_flags           1 2 4      size tiled, k = 150           -                  the sweep's own
    F summary_after_a_fed_replay                32         run, download=False           one date           -
    G backtest_portfolios_grid_on_the_tiled...  2 + 4      grid tiled, sizes 100, 150    what the pack misses  -

Measured on an MI355X (profiles/replay_batch_large_gpu_tests.txt).  C, max |device - truth| / tolerance: k = 513 1.136e-06,
k = 1025 1.870e-06, k = 2047 1.321e-06 (the rows are patches of gross exposure 2 over 10 trading days: an ulp or two).  The
slowest case of this file takes 0.34 s (A at k = 2047, which makes the source), the slowest of tests/test_gpu_replay_large.py
in the same run 1.19 s.

Sensitivity, once, in a scratch build: three one-line mutations of csrc/backtest_replay.hip - wrong arithmetic, every read in
bounds - each run against this file alone.
  (i) the late form loads the source row even where the date is patched: 12 of 22 fail.  B at all three k, C at all three k
      (before the truth is consulted), the summary F and the four-class size sweep on the bytes against the yardstick; D
      k513-middle, k1025-middle, k1025-date0, k1025-last on the patched twin's bytes.  The k = 40 cases of D pass: the early form.
      tests/test_gpu_replay_batch.py: nothing in it patches a late-form portfolio, so none of its tests can see this.
 (ii) the patch cursor does not advance after a patched date: 8 of 22 fail.  B at all three k, the four-class size sweep and G
      (the product function's own patches) on the bytes; C at all three k on the status (the date after the first patch reads
      the flagged window).  In tests/test_gpu_replay_batch.py the two-class patch test (k = 40, 130) and the product test
      (sizes 5, 8) hold portfolios with two patches or more: the small-k ones alone.
(iii) the status read at s_off + j instead of s_off + j s_stride: 10 of 22 fail, all on the status.  B at all three k (the
      portfolio that holds one row on every date walks into the flagged window), D in all six cases (the neighbours), the
      tiled size sweep's own flags (a flagged size runs on).  In tests/test_gpu_replay_batch.py the flagged-row test (k = 40)
      has such neighbours: a small-k one alone; its sweeps' statuses are all OK, so their strides do not show there.
What the earlier file would have caught is read off its cases, not run: under (iii) its neighbours' reads would leave the
status array.
"""
import numpy as np
import pandas as pd
import pytest

from incorporating_different_sources_amd import _native, synthetic

import _replay_cases as rc
from _replay_batch_cases import GAMMA, _common, _jeffreys_batch, _scales, _yardstick
from _replay_cases import _same_bytes, _universes
from _replay_reference import replay_reference_arrays

pytestmark = pytest.mark.gpu

OK = _native.STATUS_OK
POISONED = 4                                   # the window of every shared source that holds a NaN
LONG = (40, 513, 1025, 2047)                   # sources of 8 windows (flagged rows, status offsets up to 7); the others have 5


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


def _rows(k):
    return k + max(24, k // 8)


@pytest.fixture(scope="module")
def sources(dev):
    """k -> a Jeffreys batch after `run`, with its download: made on first use, shared, never written again."""
    made = {}

    def get(k):
        if k not in made:
            W = 8 if k in LONG else 5
            b = _jeffreys_batch(dev, np.random.default_rng(5000 + k), k, W, n_r=_rows(k), poison=(POISONED, 11, 5))
            b.run()
            weights, status, _ = b.download(want_aux=False)
            clean = np.arange(W) != POISONED
            assert (status[clean] == OK).all() and status[POISONED] != OK, status
            assert np.isfinite(weights[clean]).all() and weights[clean].any(axis=1).all()
            made[k] = dict(b=b, weights=weights, status=status, W=W)
        return made[k]

    yield get
    for src in made.values():
        src["b"].close()


def _universe(rng, R, k, n, scaling=None, cost=None):
    """One universe table [R x k] whose prefix every one of the n portfolios holds."""
    K = 2 * k + 7
    return dict(cols=_universes(rng, R, k, K), caps=rng.lognormal(3, 1, (R, k)), u_off=np.zeros(n, dtype=np.int64),
                u_stride=np.full(n, k, dtype=np.int64), scaling=np.full(n, 5.0) if scaling is None else np.asarray(scaling, dtype=np.float64),
                cost=np.full(n, 15.0) if cost is None else np.asarray(cost, dtype=np.float64))


def _one(res, p):
    return [x[p:p + 1] for x in res]


def _i64(a):
    return np.asarray(a, dtype=np.int64)


# ---- A. the run source at the class edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [257, 1024, 1025, 2047])
def test_run_source_at_the_class_edges(dev, sources, k):
    src = sources(k)
    b, weights, status = src["b"], src["weights"], src["status"]
    rng = np.random.default_rng(5100 + k)
    R = 4
    common = _common(rng, R, 2 * k + 7)
    ks = [k, k, k]
    universe = _universe(rng, R, k, 3, scaling=[1.0, 5.0, 2.5], cost=[15.0, 0.0, 35.0])
    zeros, stride = np.zeros(3, dtype=np.int64), np.full(3, k, dtype=np.int64)
    gammas = [None, 3.0, None]
    got = b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_off=zeros, w_stride=stride, s_off=zeros,
                   s_stride=np.ones(3, dtype=np.int64), w_scale=_scales(gammas), **common, **universe)
    want = _yardstick(dev, common, ks, universe, weights, zeros, stride, gammas)
    assert (got[3] == 0).all() and (got[4] == -1).all()
    assert np.isfinite(got[0][:, 1:]).all() and np.isfinite(got[1][:, 1:]).all()
    assert _same_bytes(got, want)
    assert got[0][0].tobytes() != got[0][1].tobytes() != got[0][2].tobytes()
    again = b.download(want_aux=False)
    assert again[0].tobytes() == weights.tobytes() and again[1].tobytes() == status.tobytes()


# ---- B. patches in the late form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [513, 1025, 2047])
def test_patches_in_the_late_form(dev, sources, k):
    """Portfolio -> patched dates: 0 -> date 0; 1 -> the last; 2 -> two adjacent; 3 -> every date; 4, 5 -> none (5 holds the row
    of date 1 on every date).  One patch row holds NaN, -0.0 and 0.0.  patch_ld = k, then k + 3 with 1e300 in the columns
    beyond k: a row read at the wrong stride would show."""
    src = sources(k)
    b, weights = src["b"], src["weights"]
    rng = np.random.default_rng(5200 + k)
    R, n = 4, 6
    patched = {0: [0], 1: [R - 1], 2: [1, 2], 3: list(range(R))}
    port = np.array([p for p in sorted(patched) for _ in patched[p]], dtype=np.int64)
    date = np.array([j for p in sorted(patched) for j in patched[p]], dtype=np.int32)
    rows = rc.gross_two(rng.normal(0.01, 0.2, (port.size, k)))
    q = int(np.flatnonzero((port == 2) & (date == 2))[0])
    rows[q, 3], rows[q, 7], rows[q, k - 1] = np.nan, -0.0, 0.0
    common = _common(rng, R, 2 * k + 7)
    gammas = [3.0, None, 7.0, None, 3.0, None]
    ks = [k] * n
    universe = _universe(rng, R, k, n, scaling=[5.0, 1.0, 2.5, 5.0, 1.0, 2.5], cost=[15.0, 0.0, 35.0, 15.0, 5.0, 0.0])
    where = dict(w_off=_i64([0, 0, 0, 0, 0, k]), w_stride=_i64([k, k, k, k, k, 0]), s_off=_i64([0, 0, 0, 0, 0, 1]),
                 s_stride=_i64([1, 1, 1, 1, 1, 0]))
    call = dict(k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), **where, **common, **universe)
    got = b.replay(_native.REPLAY_SRC_RUN, patches=(port, date, rows), **call)
    want = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas, (port, date, rows))
    assert (got[3] == 0).all() and (got[4] == -1).all()
    assert _same_bytes(got, want)
    # the patches matter: without them the patched portfolios differ, the others do not
    bare = b.replay(_native.REPLAY_SRC_RUN, **call)
    assert _same_bytes(bare, _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas))
    for p in range(n):
        assert (got[0][p].tobytes() != bare[0][p].tobytes()) == (p in patched), p
    # patch rows wider than k
    wide = np.concatenate([rows, np.full((port.size, 3), 1e300)], axis=1)
    assert _same_bytes(b.replay(_native.REPLAY_SRC_RUN, patches=(port, date, wide), **call), want)


# ---- C. the fed kernel against the 80-bit truth, every row a patch -------------------------------------------------------
@pytest.mark.parametrize("k", [513, 1025, 2047])
def test_every_row_a_patch_against_the_truth(dev, sources, k):
    """Two portfolios whose source rows include the flagged window (0: windows 1 .. 4, the flagged one on the last date; 1: the
    flagged window on every date), every date patched: a patched date reads neither the source row nor its status."""
    src = sources(k)
    b, weights, status = src["b"], src["weights"], src["status"]
    assert status[POISONED] != OK
    rng = np.random.default_rng(5300 + k)
    R, n = 4, 2
    common = _common(rng, R, 2 * k + 7)
    port, date = np.repeat(np.arange(n, dtype=np.int64), R), np.tile(np.arange(R, dtype=np.int32), n)
    rows = rc.gross_two(rng.normal(0.01, 0.3, (n * R, k)))
    # the three conditions of the tolerance's derivation
    assert np.allclose(np.abs(rows).sum(axis=1), rc.GROSS, rtol=1e-12, atol=0)
    assert int(np.diff(common["reb_day"]).max()) <= 23
    finite = common["S"][np.isfinite(common["S"])]
    assert abs(finite.mean() - 0.0005) < 1e-3 and abs(finite.std() - 0.02) < 2e-3 and np.abs(finite).max() < 0.2
    ks = [k] * n
    scaling, cost = [5.0, 2.5], [15.0, 35.0]
    universe = _universe(rng, R, k, n, scaling=scaling, cost=cost)
    w_off, w_stride = _i64([k, POISONED * k]), _i64([k, 0])
    got = b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_off=w_off, w_stride=w_stride, s_off=_i64([1, POISONED]),
                   s_stride=_i64([1, 0]), w_scale=_scales([3.0, None]), patches=(port, date, rows), **common, **universe)
    returns, turnover, metrics, rstatus, bad_day = got
    assert (rstatus == 0).all() and (bad_day == -1).all()
    assert _same_bytes(got, _yardstick(dev, common, ks, universe, weights, w_off, w_stride, [3.0, None], (port, date, rows)))
    worst = 0.0
    for p in range(n):
        truth = replay_reference_arrays(common["S"], common["rf_daily"], common["reb_day"], rows[p * R:(p + 1) * R], universe["cols"],
                                        universe["caps"], scaling[p], cost[p])
        mine = (returns[p, 1:], turnover[p, 1:], metrics[p])
        r = rc.ratio(mine, truth, f"k={k} portfolio {p}")
        assert rc.selections_equal(mine[2], truth[2]), f"k={k} portfolio {p}: max_long / max_short"
        assert r <= 1, f"k={k} portfolio {p}: device vs truth at {r:.3g} of the tolerance"
        worst = max(worst, r)
    print(f"every row a patch, k = {k}: max |device - truth| / tolerance = {worst:.3e}")


# ---- D. flagged source rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,first,R", [(513, 0, 6), (1025, 0, 6), (40, POISONED, 4), (1025, POISONED, 4), (40, POISONED - 3, 4),
                                       (1025, POISONED - 3, 4)],
                         ids=["k513-middle", "k1025-middle", "k40-date0", "k1025-date0", "k40-last", "k1025-last"])
def test_a_flagged_row_ends_the_portfolio_that_reads_it(dev, sources, k, first, R):
    """0: a neighbour that holds the row of window 0 on every date; 1: reads windows first .. first + R - 1, the flagged one among
    them; 2: as 1, the flagged date patched; 3: another neighbour, the row of window 1 on every date."""
    src = sources(k)
    b, weights, status = src["b"], src["weights"], src["status"]
    rng = np.random.default_rng(5400 + 10 * k + first)
    flagged = status[first:first + R] != OK
    assert flagged.sum() == 1
    jb = int(np.flatnonzero(flagged)[0])
    assert jb == POISONED - first
    common = _common(rng, R, 2 * k + 7)
    D = common["S"].shape[0]
    db = int(common["reb_day"][jb])
    n = 4
    universe = _universe(rng, R, k, n)
    w_off, w_stride = _i64([0, first * k, first * k, k]), _i64([0, k, k, 0])
    s_off, s_stride = _i64([0, first, first, 1]), _i64([0, 1, 1, 0])
    patches = (_i64([2]), np.array([jb], dtype=np.int32), rc.gross_two(rng.normal(0.01, 0.2, (1, k))))
    ks = [k] * n
    got = b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_off=w_off, w_stride=w_stride, s_off=s_off,
                   s_stride=s_stride, patches=patches, **common, **universe)
    want = _yardstick(dev, common, ks, universe, weights, w_off, w_stride, None, patches)
    returns, turnover, metrics, rstatus, bad_day = got
    assert rstatus.tolist() == [0, _native.REPLAY_BAD_WEIGHTS, 0, 0]
    assert bad_day.tolist() == [-1, db, -1, -1]
    for p in (0, 2, 3):                                               # the neighbours and the patched twin: untouched
        assert _same_bytes(_one(got, p), _one(want, p)), p
        assert np.isfinite(returns[p, 1:]).all() and np.isfinite(turnover[p, 1:]).all()
    # the portfolio that read the flagged row: NaN from there on, the yardstick's bytes before
    assert np.isnan(returns[1, db:]).all() and np.isnan(turnover[1, jb:]).all() and np.isnan(metrics[1, jb:]).all()
    assert returns[1, :db].tobytes() == want[0][1, :db].tobytes()
    assert turnover[1, :jb].tobytes() == want[1][1, :jb].tobytes()
    assert metrics[1, :jb].tobytes() == want[2][1, :jb].tobytes()
    assert np.isfinite(returns[1, 1:db]).all() and np.isfinite(turnover[1, 1:jb]).all() and np.isfinite(metrics[1, :jb]).all()
    if jb == 0:
        assert db == 0 and np.isnan(returns[1]).all() and np.isnan(turnover[1]).all() and np.isnan(metrics[1]).all()
    if jb == R - 1:
        assert db == D - 3 and returns[1, :db].size == D - 3 and turnover[1, :jb].size == R - 1


# ---- E. tiled sweeps as sources -------------------------------------------------------------------------------------------
def _entries_call(rng, R, k, per_window, ks, gammas=None):
    """Every entry of a sweep's [W x per_window x k] results as a portfolio: (universe, where)."""
    n = per_window
    assert len(ks) == n
    at = np.arange(n, dtype=np.int64)
    scaling = [(1.0, 5.0, 2.5)[e % 3] for e in range(n)]
    cost = [(15.0, 0.0, 35.0, 5.0)[e % 4] for e in range(n)]
    where = dict(w_off=at * k, w_stride=np.full(n, n * k, dtype=np.int64), s_off=at, s_stride=np.full(n, n, dtype=np.int64))
    return _universe(rng, R, k, n, scaling=scaling, cost=cost), where


def test_every_tiled_source_constant_reaches_its_own_buffer(dev):
    """A conjugate batch at k = 144 with the four tiled sweeps on it (P = 2 priors, sizes [100, 144], 2 lengths); every entry of
    every sweep is a portfolio of that source's call."""
    k, N, W, P, sizes = 144, 312, 4, 2, [100, 144]
    S, L = len(sizes), 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=77200, hf_days=2)
    n_r = inp["n_r"]
    rng = np.random.default_rng(77200)
    Nl = np.array([101, N], dtype=np.int32)
    rows = np.tile(np.array([100, n_r], dtype=np.int32), (W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, L))
    w0 = np.zeros((W, P, S, k))
    for s, ks in enumerate(sizes):
        w0[:, :, s, :ks] = rng.dirichlet(np.ones(ks), size=(W, P))
    common = _common(rng, W, 2 * k + 7)
    with dev.batch("conjugate", k, N, n_r, GAMMA, W, inp["m"]) as b:
        b.upload(inp["panel"], start=inp["start"][:W], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"][:W], w0=inp["w0"][:W],
                 n0=inp["n0"][:W])
        full, last = np.ascontiguousarray(w0[:, :, -1]), np.ascontiguousarray(n0[:, :, 1])
        down = {"grid": b.grid_sweep_tiled(sizes, Nl, rows, n0, w0, want_aux=False),
                "window": b.window_sweep_tiled(Nl, rows, n0, full, want_aux=False),
                "size": b.size_sweep_tiled(sizes, last, w0, want_aux=False),
                "prior": b.prior_sweep_tiled(last, full, want_aux=False)}
        seen = {}
        for source, name, per_window, ks, entry in (
                (_native.REPLAY_SRC_GRID_SWEEP, "grid", P * L * S, sizes * (P * L), (1 * L + 0) * S + 0),
                (_native.REPLAY_SRC_WINDOW_SWEEP, "window", P * L, [k] * (P * L), 1 * L + 0),
                (_native.REPLAY_SRC_SIZE_SWEEP, "size", P * S, sizes * P, 1 * S + 0),
                (_native.REPLAY_SRC_PRIOR_SWEEP, "prior", P, [k] * P, 1)):
            weights, status, _ = down[name]
            assert (status == OK).all(), name
            assert weights.size == W * per_window * k and np.isfinite(weights).all(), name
            universe, where = _entries_call(np.random.default_rng(77201), W, k, per_window, ks)
            got = b.replay(source, k=np.array(ks, dtype=np.int32), **where, **common, **universe)
            want = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"])
            assert (got[3] == 0).all() and np.isfinite(got[0][:, 1:]).all(), name
            assert _same_bytes(got, want), name
            assert len({got[0][p].tobytes() for p in range(per_window)}) == per_window, name
            # prior 1 with: the shorter length and the smaller size; the shorter length; the smaller size; neither
            seen[name] = got[1][entry].tobytes() + got[2][entry].tobytes()
        assert len(set(seen.values())) == 4


def test_tiled_grid_sweep_two_classes(dev):
    """A Jeffreys grid sweep at k = 520, sizes [100, 520], two lengths: four entries, 2 and 16 slots per lane in one call, both
    on the prefix of one universe table."""
    k, W, sizes = 520, 4, [100, 520]
    rng = np.random.default_rng(5500)
    n_r = _rows(k)
    Nl = np.array([n_r - 12, n_r], dtype=np.int32)
    with _jeffreys_batch(dev, rng, k, W, n_r=n_r) as b:
        weights, status, _ = b.grid_sweep_tiled(sizes, Nl, np.tile(Nl, (W, 1)), want_aux=False)
        assert (status == OK).all() and np.isfinite(weights).all()
        ks = sizes * 2
        gammas = [None, 3.0, 7.0, None]
        universe, where = _entries_call(rng, W, k, 4, ks)
        common = _common(rng, W, 2 * k + 7)
        got = b.replay(_native.REPLAY_SRC_GRID_SWEEP, k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), **where, **common,
                       **universe)
        want = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas)
        assert (got[3] == 0).all() and (got[4] == -1).all() and np.isfinite(got[0][:, 1:]).all()
        assert _same_bytes(got, want)
        assert len({got[0][p].tobytes() for p in range(4)}) == 4


def test_tiled_size_sweep_four_classes(dev):
    """A Jeffreys size sweep at k = 1100, sizes [40, 300, 600, 1100]: ten portfolios interleaved over the sizes (1, 8, 16 and 32
    slots per lane: the launch order is not the portfolios' order), some of every class patched."""
    k, W, sizes = 1100, 4, [40, 300, 600, 1100]
    R = W
    rng = np.random.default_rng(5600)
    with _jeffreys_batch(dev, rng, k, W, n_r=_rows(k)) as b:
        weights, status, _ = b.size_sweep_tiled(sizes, want_aux=False)
        assert (status == OK).all() and np.isfinite(weights).all()
        ks = [1100, 40, 600, 300, 40, 1100, 300, 600, 40, 1100]
        n, S = len(ks), len(sizes)
        s_of = _i64([sizes.index(x) for x in ks])
        patched = {0: [0, 1], 1: [R - 1], 2: list(range(R)), 3: [2], 4: [0], 6: [1, 2], 7: [R - 1], 8: [1, 3]}     # 5 and 9: none
        port = np.array([p for p in sorted(patched) for _ in patched[p]], dtype=np.int64)
        date = np.array([j for p in sorted(patched) for j in patched[p]], dtype=np.int32)
        rows = np.full((port.size, k), 1e300)                             # beyond a portfolio's own k: never read
        for q, p in enumerate(port):
            rows[q, :ks[p]] = rc.gross_two(rng.normal(0.01, 0.2, ks[p]))
        gammas = [3.0, None, 7.0, 3.0, 7.0, None, 3.0, None, 3.0, 7.0]
        universe = _universe(rng, R, k, n, scaling=[(1.0, 5.0, 2.5)[p % 3] for p in range(n)])
        common = _common(rng, R, 2 * k + 7)
        where = dict(w_off=s_of * k, w_stride=np.full(n, S * k, dtype=np.int64), s_off=s_of, s_stride=np.full(n, S, dtype=np.int64))
        call = dict(k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), **where, **common, **universe)
        got = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, patches=(port, date, rows), **call)
        want = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas, (port, date, rows))
        assert (got[3] == 0).all() and (got[4] == -1).all() and np.isfinite(got[0][:, 1:]).all()
        assert _same_bytes(got, want)
        bare = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, **call)
        assert _same_bytes(bare, _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas))
        for p in range(n):
            assert (got[0][p].tobytes() != bare[0][p].tobytes()) == (p in patched), p
        # a patch row narrower than the widest portfolio: patch_ld = 40 serves the k = 40 portfolios
        only40 = np.isin(port, [p for p in range(n) if ks[p] == 40])
        narrow = (port[only40], date[only40], np.ascontiguousarray(rows[only40, :40]))
        got40 = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, patches=narrow, **call)
        assert _same_bytes(got40, _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas, narrow))
        assert not _same_bytes(got40, got) and not _same_bytes(got40, bare)


def test_the_tiled_size_sweeps_own_flags(dev):
    """A NaN in column 100 of window 2: the tiled size sweep flags every size that holds the column and some smaller ones.  Which
    ones is read from the sweep's own status."""
    k, W, sizes, jw, col = 150, 4, [40, 64, 80, 150], 2, 100
    R, S = W, 4
    rng = np.random.default_rng(5700)
    with _jeffreys_batch(dev, rng, k, W, poison=(jw, 11, col)) as b:
        weights, status, _ = b.size_sweep_tiled(sizes, want_aux=False)
        status = status.reshape(W, S)
        flagged = status[jw] != OK
        assert (status[np.arange(W) != jw] == OK).all(), status
        assert flagged.any() and not flagged.all(), status
        below = [s for s in range(S) if sizes[s] <= col]                   # sizes that do not hold the column
        assert any(flagged[s] for s in below) and not all(flagged[s] for s in below), status
        assert all(np.isfinite(weights[jw, 0, s, :sizes[s]]).all() for s in range(S) if not flagged[s])
        universe, where = _entries_call(rng, R, k, S, sizes)
        common = _common(rng, R, 2 * k + 7)
        db = int(common["reb_day"][jw])
        got = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, k=np.array(sizes, dtype=np.int32), **where, **common, **universe)
        want = _yardstick(dev, common, sizes, universe, weights, where["w_off"], where["w_stride"])
        returns, turnover, metrics, rstatus, bad_day = got
        for s in range(S):
            if not flagged[s]:
                assert rstatus[s] == 0 and bad_day[s] == -1 and np.isfinite(returns[s, 1:]).all(), s
                assert _same_bytes(_one(got, s), _one(want, s)), s
                continue
            assert rstatus[s] == _native.REPLAY_BAD_WEIGHTS and bad_day[s] == db, s
            assert np.isnan(returns[s, db:]).all() and np.isnan(turnover[s, jw:]).all() and np.isnan(metrics[s, jw:]).all(), s
            assert returns[s, :db].tobytes() == want[0][s, :db].tobytes() and np.isfinite(returns[s, 1:db]).all(), s
            assert turnover[s, :jw].tobytes() == want[1][s, :jw].tobytes(), s
            assert metrics[s, :jw].tobytes() == want[2][s, :jw].tobytes(), s


# ---- F. the summary after a fed replay in the late form -----------------------------------------------------------------------
def test_summary_after_a_fed_replay(dev, sources):
    k = 1025
    src = sources(k)
    b, weights = src["b"], src["weights"]
    rng = np.random.default_rng(5800)
    R, n = 4, 3
    common = _common(rng, R, 2 * k + 7)
    D = common["S"].shape[0]
    ks = [k] * n
    universe = _universe(rng, R, k, n, scaling=[1.0, 5.0, 2.5], cost=np.zeros(n))
    gammas = [None, 3.0, 7.0]
    where = dict(w_off=np.zeros(n, dtype=np.int64), w_stride=np.full(n, k, dtype=np.int64), s_off=np.zeros(n, dtype=np.int64),
                 s_stride=np.ones(n, dtype=np.int64))
    patches = (_i64([2]), np.array([1], dtype=np.int32), rc.gross_two(rng.normal(0.01, 0.2, (1, k))))
    cost_bp, rf_excess = np.array([0.0, 15.0, 35.0]), np.full(D, 1e-4)
    assert b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), patches=patches, download=False,
                    **where, **common, **universe) is None
    fed, fed_status = dev.replay_summary(cost_bp, rf_excess)
    kept = dev._replay_download(n, D, R)                                  # (download=False copied nothing; it is all still there)
    assert (kept[3] == 0).all() and np.isfinite(kept[0][:, 1:]).all()
    assert fed.shape[:2] == (n, 3) and len({fed[p, c].tobytes() for p in range(n) for c in range(3)}) == 3 * n
    before = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas, patches)
    assert _same_bytes(before, kept)
    host_fed, host_fed_status = dev.replay_summary(cost_bp, rf_excess)
    assert host_fed.tobytes() == fed.tobytes() and host_fed_status.tobytes() == fed_status.tobytes()
    assert _same_bytes(dev._replay_download(n, D, R), before)
    # and the fed replay's own download is the same before and after its summary
    b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), patches=patches, download=False,
             **where, **common, **universe)
    first = dev._replay_download(n, D, R)
    again, again_status = dev.replay_summary(cost_bp, rf_excess)
    assert again.tobytes() == fed.tobytes() and again_status.tobytes() == fed_status.tobytes()
    assert _same_bytes(dev._replay_download(n, D, R), first) and _same_bytes(first, kept)


# ---- G. the product function on the tiled grid sweep -----------------------------------------------------------------------
def _spec(k, N, gamma):
    return {"weighting_strategy": "jeffreys", "size": k, "risk_aversion": gamma, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": None, "display_name": f"jeffreys_{k}_{N}_{gamma}"}


def test_backtest_portfolios_grid_on_the_tiled_grid_sweep(monkeypatch):
    """Sizes 100 and 150 (the larger above the one-wave sweeps' bound), windows 160 and 175, 170 tickers, 6 daily dates."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    monkeypatch.setattr(pc, "GRID_SWEEP_TILED", True)
    md, _ = synthetic.make_market_data(n_tickers=170, n_days=260, seed=20240095)
    days = md["stock_prices_df"].index
    prices = md["stock_prices_df"].copy()                                 # a late-listed large cap, as in the small product test:
    prices.loc[prices.index < days[78], md["stock_market_caps_df"].loc[days[250]].idxmax()] = np.nan
    md = dict(md, stock_prices_df=prices)                                 # the shorter window misses 2 of the 6 dates, at both sizes
    sizes, windows = [100, 150], [160, 175]
    assert sizes[-1] > _native.sweep_max_assets()
    specs = [_spec(100, 160, 5), _spec(100, 175, 10), _spec(150, 160, 10), _spec(150, 175, 5)]
    start, end = pd.Timestamp(days[250]), pd.Timestamp(days[255])
    trading = [pd.Timestamp(ts) for ts in days if start <= ts <= end]
    reb = pc.rebalancing_schedule(trading, "daily")
    # on the CPU, before any device call: the pack serves at least one date of every (size, length)
    batch.clear_panel_cache()
    mask = batch.pack_windows_grid(reb, specs[0], sizes, windows, md)[5]
    assert mask.shape == (len(reb), 2, 2) and mask.any(axis=0).all(), mask.sum(axis=0)
    assert not mask[:, :, 0].all(axis=0).any() and mask[:, :, 1].all(), mask.sum(axis=0)       # patches at both sizes
    batch.clear_panel_cache()
    tiled = []
    real = _native.Batch.grid_sweep_tiled
    monkeypatch.setattr(_native.Batch, "grid_sweep_tiled", lambda self, *a, **kw: (tiled.append(kw.get("want_weights")), real(self, *a, **kw))[1])
    monkeypatch.setattr(_native.Batch, "grid_sweep", lambda *a, **kw: pytest.fail("the sweep did not run tiled"))
    found = pc.calculate_weights_for_grid(reb, specs, md)
    assert tiled == [True]
    tickers = batch.panels_for(md, "daily").tickers
    want = pc.replay_backtests_device(trading, reb, [(res[0], res[2], res[3], sp) for res, sp in zip(found, specs)], md,
                                      tickers=tickers)
    batch.clear_panel_cache()
    monkeypatch.setattr(_native.Device, "replay", lambda *a, **kw: pytest.fail("the host-fed replay ran"))
    downloads = []
    real_download = _native.Device._replay_download
    monkeypatch.setattr(_native.Device, "_replay_download", lambda self, *a: (downloads.append(a), real_download(self, *a))[1])
    got = pc.backtest_portfolios_grid(specs, start, end, md)
    assert tiled == [True, False]                                         # one more tiled sweep, its weights never downloaded
    assert downloads == [(len(specs), len(trading), len(reb))]            # results came down, once
    assert list(got) == [sp["display_name"] for sp in specs]
    for sp, w in zip(specs, want):
        g = got[sp["display_name"]]
        for key in ("portfolio_simple_returns_series", "portfolio_turnover_series"):
            assert g[key].index.equals(w[key].index) and g[key].name == w[key].name == sp["display_name"]
            assert g[key].dtype == w[key].dtype
            assert g[key].to_numpy().tobytes() == w[key].to_numpy().tobytes(), f"{sp['display_name']} {key}"
            assert np.isfinite(g[key].to_numpy()).all()
        gm, wm = g["portfolio_weights_metrics_df"], w["portfolio_weights_metrics_df"]
        assert gm.index.equals(wm.index) and list(gm.columns) == list(wm.columns) and (gm.dtypes == wm.dtypes).all()
        assert gm.to_numpy().tobytes() == wm.to_numpy().tobytes(), sp["display_name"]
    batch.clear_panel_cache()
