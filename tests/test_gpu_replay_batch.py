"""The device-fed backtest replay (-m gpu): `tp_replay_run_batch` / `Batch.replay` read the weights where a batch's run or
sweep left them on the device, scale them per portfolio, substitute patch rows and honour the source's statuses.

The yardstick of every comparison is the merged path, never the code under test: download the source, apply scale and patches
in numpy with the host's own expression `1.0 / g * w`, call `Device.replay` on the dense rows.  The comparisons are byte for
byte: both sides run the same daily loop on the same weight bits (one IEEE multiplication on either side), and a portfolio's
results do not depend on how its rows are addressed.

Shapes: the smallest that reach every form - k = 5, 64, 65 (1 and 2 slots per lane), 512 (the last size whose rebalancing
inputs are requested ahead of the day's reductions) and 513 (the first that requests them after the mark to market; its source
is a large-k run); two launch classes in one call (k = 40 and 130); R = 4 .. 6 rebalancing dates."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from incorporating_different_sources_amd import _native, synthetic

from _replay_batch_cases import GAMMA, _common, _jeffreys_batch, _scales, _yardstick
from _replay_cases import _same_bytes, _universes

pytestmark = pytest.mark.gpu

INVALID = _native.ERR_INVALID


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


# ---- A. the run source, every launch form ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 64, 65, 512, 513])
def test_run_source_at_every_launch_form(dev, k):
    rng = np.random.default_rng(4100 + k)
    W = R = 4
    with _jeffreys_batch(dev, rng, k, W) as b:
        b.run()
        weights, status, _ = b.download(want_aux=False)
        assert (status == _native.STATUS_OK).all(), status
        assert np.isfinite(weights).all() and weights.any()
        K = 2 * k + 7
        common = _common(rng, R, K)
        ks = [k, k, k]
        universe = dict(cols=_universes(rng, R, k, K), caps=rng.lognormal(3, 1, (R, k)), u_off=np.zeros(3, dtype=np.int64),
                        u_stride=np.full(3, k, dtype=np.int64), scaling=np.array([1.0, 5.0, 2.5]), cost=np.array([15.0, 0.0, 35.0]))
        zeros, stride = np.zeros(3, dtype=np.int64), np.full(3, k, dtype=np.int64)
        gammas = [None, 3.0, None]
        got = b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_off=zeros, w_stride=stride, s_off=zeros,
                       s_stride=np.ones(3, dtype=np.int64), w_scale=_scales(gammas), **common, **universe)
        want = _yardstick(dev, common, ks, universe, weights, zeros, stride, gammas)
        assert (got[3] == 0).all() and (got[4] == -1).all()
        assert np.isfinite(got[0][:, 1:]).all() and np.isfinite(got[1][:, 1:]).all()
        assert _same_bytes(got, want)
        again = b.download(want_aux=False)
        assert again[0].tobytes() == weights.tobytes() and again[1].tobytes() == status.tobytes()


# ---- B. the grid sweep's results in place, and every other source constant ---------------------------------------------
GRID = dict(k=24, N=130, W=5, P=2, sizes=[8, 24])


@pytest.fixture(scope="module")
def grid(dev):
    """A conjugate batch with a grid sweep, a window sweep, a size sweep and a prior sweep on it; the downloads of each."""
    k, N, W, P, sizes = GRID["k"], GRID["N"], GRID["W"], GRID["P"], GRID["sizes"]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=77100)
    n_r = inp["n_r"]
    rng = np.random.default_rng(77100)
    Nl = np.array([64, N], dtype=np.int32)
    rows = np.tile(np.array([63, n_r], dtype=np.int32), (W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, 2))
    w0 = np.zeros((W, P, len(sizes), k))
    for s, ks in enumerate(sizes):
        w0[:, :, s, :ks] = rng.dirichlet(np.ones(ks), size=(W, P))
    b = dev.batch("conjugate", k, N, n_r, GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"][:W], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"][:W], w0=inp["w0"][:W],
             n0=inp["n0"][:W])
    prior_args = (np.ascontiguousarray(n0[:, :, 1]), np.ascontiguousarray(w0[:, :, -1]))
    out = {"b": b, "L": 2, "prior_args": prior_args,
           "grid": b.grid_sweep(sizes, Nl, rows, n0, w0),
           "window": b.window_sweep(Nl, rows, n0, np.ascontiguousarray(w0[:, :, -1])),
           "size": b.size_sweep(sizes, np.ascontiguousarray(n0[:, :, 1]), w0),
           "prior": b.prior_sweep(*prior_args)}
    for name in ("grid", "window", "size", "prior"):
        assert (out[name][1] == _native.STATUS_OK).all(), name
    K = 2 * k + 7
    out["common"] = _common(rng, W, K)
    out["cols"], out["caps"] = _universes(rng, W, k, K), rng.lognormal(3, 1, (W, k))
    yield out
    b.close()


def _grid_call(grid):
    """All 8 (prior, length, size) entries as portfolios of one call; they share the prefix of one universe table."""
    k, P, L, sizes = GRID["k"], GRID["P"], grid["L"], GRID["sizes"]
    S = len(sizes)
    entries = [(p, l, s) for p in range(P) for l in range(L) for s in range(S)]
    n = len(entries)
    at = np.array([(p * L + l) * S + s for p, l, s in entries], dtype=np.int64)
    ks = [sizes[s] for _, _, s in entries]
    universe = dict(cols=grid["cols"], caps=grid["caps"], u_off=np.zeros(n, dtype=np.int64), u_stride=np.full(n, k, dtype=np.int64),
                    scaling=np.full(n, 5.0), cost=np.full(n, 15.0))
    where = dict(w_off=at * k, w_stride=np.full(n, P * L * S * k, dtype=np.int64), s_off=at,
                 s_stride=np.full(n, P * L * S, dtype=np.int64))
    return ks, universe, where


def test_grid_sweep_source_in_place(dev, grid):
    ks, universe, where = _grid_call(grid)
    got = grid["b"].replay(_native.REPLAY_SRC_GRID_SWEEP, k=np.array(ks, dtype=np.int32), **where, **grid["common"], **universe)
    want = _yardstick(dev, grid["common"], ks, universe, grid["grid"][0], where["w_off"], where["w_stride"])
    assert (got[3] == 0).all() and np.isfinite(got[0][:, 1:]).all()
    assert _same_bytes(got, want)
    assert len({got[0][p].tobytes() for p in range(len(ks))}) == len(ks)      # eight different portfolios


def test_every_source_constant_reaches_its_own_buffer(dev, grid):
    k, P, L, S, W = GRID["k"], GRID["P"], grid["L"], len(GRID["sizes"]), GRID["W"]
    seen = []
    for source, name, per_window, entry, kp in (
            (_native.REPLAY_SRC_WINDOW_SWEEP, "window", P * L, 1 * L + 0, k),          # prior 1, the shorter length
            (_native.REPLAY_SRC_SIZE_SWEEP, "size", P * S, 1 * S + 0, GRID["sizes"][0]),   # prior 1, the smaller size
            (_native.REPLAY_SRC_PRIOR_SWEEP, "prior", P, 1, k)):
        weights = grid[name][0]
        assert weights.size == W * per_window * k
        ks = [kp, kp]
        universe = dict(cols=grid["cols"], caps=grid["caps"], u_off=np.zeros(2, dtype=np.int64), u_stride=np.full(2, k, dtype=np.int64),
                        scaling=np.full(2, 5.0), cost=np.full(2, 15.0))
        at = np.array([0, entry], dtype=np.int64)
        where = dict(w_off=at * k, w_stride=np.full(2, per_window * k, dtype=np.int64), s_off=at,
                     s_stride=np.full(2, per_window, dtype=np.int64))
        got = grid["b"].replay(source, k=np.array(ks, dtype=np.int32), **where, **grid["common"], **universe)
        want = _yardstick(dev, grid["common"], ks, universe, weights, where["w_off"], where["w_stride"])
        assert (got[3] == 0).all()
        assert _same_bytes(got, want), name
        seen.append(got[0].tobytes())
    assert len(set(seen)) == 3


# ---- C. the scale -------------------------------------------------------------------------------------------------------
def test_scale_is_the_hosts_one_over_gamma(dev):
    rng = np.random.default_rng(4300)
    k, W = 40, 5
    with _jeffreys_batch(dev, rng, k, W) as b:
        b.run()
        weights, status, _ = b.download(want_aux=False)
        assert (status == 0).all()
        K = 2 * k + 7
        common = _common(rng, W, K)
        gammas = [1.0, 3.0, 7.0]
        n = len(gammas)
        universe = dict(cols=_universes(rng, W, k, K), caps=rng.lognormal(3, 1, (W, k)), u_off=np.zeros(n, dtype=np.int64),
                        u_stride=np.full(n, k, dtype=np.int64), scaling=np.array(gammas), cost=np.full(n, 15.0))
        zeros, stride, ones = np.zeros(n, dtype=np.int64), np.full(n, k, dtype=np.int64), np.ones(n, dtype=np.int64)
        call = dict(k=np.full(n, k, dtype=np.int32), w_off=zeros, w_stride=stride, s_off=zeros, s_stride=ones, **common, **universe)
        got = b.replay(_native.REPLAY_SRC_RUN, w_scale=np.array([1.0, 1.0 / 3.0, 1.0 / 7.0]), **call)
        want = _yardstick(dev, common, [k] * n, universe, weights, zeros, stride, gammas)
        assert (got[3] == 0).all()
        assert _same_bytes(got, want)
        assert got[0][0].tobytes() != got[0][1].tobytes() != got[0][2].tobytes()
        # a scale of exactly 1.0 is no scale
        unit = b.replay(_native.REPLAY_SRC_RUN, w_scale=np.ones(n), **call)
        none = b.replay(_native.REPLAY_SRC_RUN, w_scale=None, **call)
        assert _same_bytes(unit, none)
        assert _same_bytes(none, _yardstick(dev, common, [k] * n, universe, weights, zeros, stride))


# ---- D. patches -------------------------------------------------------------------------------------------------------
def test_patches_replace_rows_unscaled_across_two_launch_classes(dev):
    """k = 40 and k = 130 portfolios interleaved (two launch classes: the launch order is not the portfolios' order), over a
    Jeffreys size sweep's results [W x 1 x 2 x 130]."""
    rng = np.random.default_rng(4400)
    k, W, sizes = 130, 6, [40, 130]
    R = W
    with _jeffreys_batch(dev, rng, k, W) as b:
        weights, status, _ = b.size_sweep(sizes, want_aux=False)
        assert (status == 0).all()
        ks = [40, 130, 40, 130, 40, 130, 40]
        n = len(ks)
        s_of = np.array([sizes.index(x) for x in ks], dtype=np.int64)
        patched = {1: [0], 2: [R - 1], 3: [2, 3], 4: list(range(R)), 6: [1, 4]}        # portfolio -> dates; 0 and 5: none
        port = np.array([p for p in sorted(patched) for _ in patched[p]], dtype=np.int64)
        date = np.array([j for p in sorted(patched) for j in patched[p]], dtype=np.int32)
        rows = rng.normal(0.01, 0.2, (port.size, k))
        q = int(np.flatnonzero((port == 6) & (date == 4))[0])
        rows[q, 3], rows[q, 7], rows[q, 11] = np.nan, -0.0, 0.0                       # ordinary data on every path
        K = 2 * k + 7
        common = _common(rng, R, K)
        gammas = [3.0, None, 7.0, 3.0, 7.0, None, 3.0]
        universe = dict(cols=_universes(rng, R, k, K), caps=rng.lognormal(3, 1, (R, k)), u_off=np.zeros(n, dtype=np.int64),
                        u_stride=np.full(n, k, dtype=np.int64), scaling=np.full(n, 5.0), cost=np.full(n, 15.0))
        where = dict(w_off=s_of * k, w_stride=np.full(n, 2 * k, dtype=np.int64), s_off=s_of, s_stride=np.full(n, 2, dtype=np.int64))
        got = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas),
                       patches=(port, date, rows), **where, **common, **universe)
        want = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas, (port, date, rows))
        assert (got[3] == 0).all() and (got[4] == -1).all()
        assert _same_bytes(got, want)
        # the patches matter: without them the patched portfolios differ, the others do not
        bare = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), **where, **common,
                        **universe)
        for p in range(n):
            assert (got[0][p].tobytes() != bare[0][p].tobytes()) == (p in patched), p
        # a patch row narrower than the widest portfolio: patch_ld = 40 serves the k = 40 portfolios
        only40 = np.isin(port, [2, 4, 6])
        narrow = (port[only40], date[only40], np.ascontiguousarray(rows[only40, :40]))
        got40 = b.replay(_native.REPLAY_SRC_SIZE_SWEEP, k=np.array(ks, dtype=np.int32), w_scale=_scales(gammas), patches=narrow,
                         **where, **common, **universe)
        want40 = _yardstick(dev, common, ks, universe, weights, where["w_off"], where["w_stride"], gammas, narrow)
        assert _same_bytes(got40, want40)


# ---- E. the statuses of the rows read -------------------------------------------------------------------------------------
def test_a_flagged_row_ends_the_portfolio_that_reads_it(dev):
    rng = np.random.default_rng(4500)
    k, W = 40, 6
    R = W
    with _jeffreys_batch(dev, rng, k, W, poison=(3, 11, 5)) as b:
        b.run()
        weights, status, _ = b.download(want_aux=False)
        flagged = status != _native.STATUS_OK
        assert flagged.any() and not flagged[0] and not flagged[1], status     # there are clean dates before the flagged one
        jb = int(np.flatnonzero(flagged)[0])
        bad_dates = [int(j) for j in np.flatnonzero(flagged)]
        K = 2 * k + 7
        common = _common(rng, R, K)
        db = int(common["reb_day"][jb])
        n = 4
        universe = dict(cols=_universes(rng, R, k, K), caps=rng.lognormal(3, 1, (R, k)), u_off=np.zeros(n, dtype=np.int64),
                        u_stride=np.full(n, k, dtype=np.int64), scaling=np.full(n, 5.0), cost=np.full(n, 15.0))
        # 0: a neighbour that holds the row of date 0 on every date; 1: reads every date; 2: as 1, the flagged dates patched;
        # 3: another neighbour, the row of date 1 on every date
        w_off = np.array([0, 0, 0, k], dtype=np.int64)
        w_stride = np.array([0, k, k, 0], dtype=np.int64)
        s_off = np.array([0, 0, 0, 1], dtype=np.int64)
        s_stride = np.array([0, 1, 1, 0], dtype=np.int64)
        port = np.full(len(bad_dates), 2, dtype=np.int64)
        date = np.array(bad_dates, dtype=np.int32)
        rows = rng.normal(0.01, 0.2, (len(bad_dates), k))
        ks = [k] * n
        got = b.replay(_native.REPLAY_SRC_RUN, k=np.array(ks, dtype=np.int32), w_off=w_off, w_stride=w_stride, s_off=s_off,
                       s_stride=s_stride, patches=(port, date, rows), **common, **universe)
        want = _yardstick(dev, common, ks, universe, weights, w_off, w_stride, None, (port, date, rows))
        returns, turnover, metrics, rstatus, bad_day = got
        assert rstatus.tolist() == [0, _native.REPLAY_BAD_WEIGHTS, 0, 0]
        assert bad_day.tolist() == [-1, db, -1, -1]
        for p in (0, 2, 3):                                               # the neighbours and the patched twin: untouched
            assert _same_bytes([x[p:p + 1] for x in got], [x[p:p + 1] for x in want]), p
        assert np.isfinite(returns[2, 1:]).all() and np.isfinite(turnover[2, 1:]).all()
        # the portfolio that read the flagged row: NaN from there on, the yardstick's bytes before
        assert np.isnan(returns[1, db:]).all() and np.isnan(turnover[1, jb:]).all() and np.isnan(metrics[1, jb:]).all()
        assert returns[1, :db].tobytes() == want[0][1, :db].tobytes()
        assert turnover[1, :jb].tobytes() == want[1][1, :jb].tobytes()
        assert metrics[1, :jb].tobytes() == want[2][1, :jb].tobytes()
        assert np.isfinite(returns[1, 1:db]).all()


# ---- F. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_are_invalid_and_keep_the_last_results(dev):
    rng = np.random.default_rng(4600)
    k, W = 12, 4
    R = W
    with _jeffreys_batch(dev, rng, k, W) as b:
        b.run()
        K = 2 * k + 7
        common = _common(rng, R, K)
        n = 2
        universe = dict(cols=_universes(rng, R, k, K), caps=rng.lognormal(3, 1, (R, k)), u_off=np.zeros(n, dtype=np.int64),
                        u_stride=np.full(n, k, dtype=np.int64), scaling=np.full(n, 5.0), cost=np.full(n, 15.0))
        good = dict(k=np.full(n, k, dtype=np.int32), w_off=np.zeros(n, dtype=np.int64), w_stride=np.full(n, k, dtype=np.int64),
                    s_off=np.zeros(n, dtype=np.int64), s_stride=np.ones(n, dtype=np.int64))
        kept = b.replay(_native.REPLAY_SRC_RUN, **good, **common, **universe)
        D = common["S"].shape[0]

        def refused(source=_native.REPLAY_SRC_RUN, patches=None, **change):
            with pytest.raises(_native.TangencyError) as err:
                b.replay(source, patches=patches, **dict(good, **change), **common, **universe)
            assert err.value.code == INVALID, err.value
            assert _same_bytes(dev._replay_download(n, D, R), kept)        # the last replay's results are still there
            return str(err.value)

        def rows(m, ld=k):
            return rng.normal(0.0, 0.1, (m, ld))

        two = lambda a, b_: np.array([a, b_])                                 # noqa: E731
        assert "unknown source" in refused(source=7)
        assert "unknown source" in refused(source=-1)
        for source in (_native.REPLAY_SRC_PRIOR_SWEEP, _native.REPLAY_SRC_SIZE_SWEEP, _native.REPLAY_SRC_WINDOW_SWEEP,
                       _native.REPLAY_SRC_GRID_SWEEP):
            assert "no results" in refused(source=source)
        # the source holds W k weights and W statuses: the last row may end exactly there, not one element later
        b.replay(_native.REPLAY_SRC_RUN, **dict(good, w_off=two(0, 0), w_stride=two(k, k)), **common, **universe)
        assert "weights" in refused(w_off=two(0, 1))
        assert "weights" in refused(w_off=two(0, W * k - k + 1), w_stride=two(k, 0))
        assert "statuses" in refused(s_off=two(0, 1))
        assert "statuses" in refused(s_off=two(0, W), s_stride=two(1, 0))
        assert refused(w_off=two(0, -1)) and refused(s_stride=two(1, -1))
        kept = b.replay(_native.REPLAY_SRC_RUN, **good, **common, **universe)
        # patches
        assert "sorted" in refused(patches=(np.array([1, 0]), np.array([0, 0], dtype=np.int32), rows(2)))          # unsorted
        assert "sorted" in refused(patches=(np.array([0, 0]), np.array([2, 1], dtype=np.int32), rows(2)))          # unsorted dates
        assert "sorted" in refused(patches=(np.array([0, 0]), np.array([1, 1], dtype=np.int32), rows(2)))          # repeated
        assert "patch_port" in refused(patches=(np.array([n]), np.array([0], dtype=np.int32), rows(1)))
        assert "patch_port" in refused(patches=(np.array([-1]), np.array([0], dtype=np.int32), rows(1)))
        assert "patch_date" in refused(patches=(np.array([0]), np.array([R], dtype=np.int32), rows(1)))
        assert "patch_date" in refused(patches=(np.array([0]), np.array([-1], dtype=np.int32), rows(1)))
        assert "patch_ld" in refused(patches=(np.array([1]), np.array([0], dtype=np.int32), rows(1, k - 1)))
        # what Python checks itself, before any library call
        with pytest.raises(ValueError):
            b.replay(_native.REPLAY_SRC_RUN, w_scale=np.ones(n + 1), **good, **common, **universe)
        with pytest.raises(ValueError):
            b.replay(_native.REPLAY_SRC_RUN, patches=(np.array([0]), np.array([0, 1], dtype=np.int32), rows(1)), **good, **common,
                     **universe)
        assert _same_bytes(dev._replay_download(n, D, R), kept)


# ---- G. nothing else moves ------------------------------------------------------------------------------------------------
def test_the_replay_leaves_the_batch_and_the_host_fed_replay_alone(dev, grid):
    b = grid["b"]
    ks, universe, where = _grid_call(grid)
    ptr = lambda a, ct: a.ctypes.data_as(ctypes.POINTER(ct))             # noqa: E731

    def download():
        out = (np.empty_like(grid["grid"][0]), np.empty_like(grid["grid"][1]), np.empty_like(grid["grid"][2]))
        assert _native.lib.tp_batch_download_grid_sweep(b._b, ptr(out[0], ctypes.c_double), ptr(out[1], ctypes.c_int32),
                                                        ptr(out[2], ctypes.c_double)) == 0
        return out

    before = download()
    assert _same_bytes(before, grid["grid"])
    dense = _yardstick(dev, grid["common"], ks, universe, grid["grid"][0], where["w_off"], where["w_stride"])
    first = b.replay(_native.REPLAY_SRC_GRID_SWEEP, k=np.array(ks, dtype=np.int32), **where, **grid["common"], **universe)
    assert _same_bytes(download(), before)
    for name, call in (("window", _native.lib.tp_batch_download_window_sweep), ("size", _native.lib.tp_batch_download_size_sweep),
                       ("prior", _native.lib.tp_batch_download_prior_sweep)):
        out = np.empty_like(grid[name][0])
        assert call(b._b, ptr(out, ctypes.c_double), None, None) == 0 and out.tobytes() == grid[name][0].tobytes(), name
    # a host-fed replay after it returns what it returns alone, and the device-fed one is repeatable
    assert _same_bytes(_yardstick(dev, grid["common"], ks, universe, grid["grid"][0], where["w_off"], where["w_stride"]), dense)
    second = b.replay(_native.REPLAY_SRC_GRID_SWEEP, k=np.array(ks, dtype=np.int32), **where, **grid["common"], **universe)
    assert _same_bytes(first, second) and _same_bytes(first, dense)
    # want_weights=False: the sweep's weights stay on the device and are the same
    kept = b.prior_sweep(*grid["prior_args"], want_aux=False, want_weights=False)
    assert kept[0] is None and kept[2] is None and kept[1].tobytes() == grid["prior"][1].tobytes()
    out = np.empty_like(grid["prior"][0])
    assert _native.lib.tp_batch_download_prior_sweep(b._b, ptr(out, ctypes.c_double), None, None) == 0
    assert out.tobytes() == grid["prior"][0].tobytes()


# ---- H. the product function ------------------------------------------------------------------------------------------------
def _spec(k, N, gamma):
    return {"weighting_strategy": "jeffreys", "size": k, "risk_aversion": gamma, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": None, "display_name": f"jeffreys_{k}_{N}_{gamma}"}


def test_backtest_portfolios_grid_equals_the_download_and_replay_path(monkeypatch):
    """A late-listed large cap: for 20 of the 36 daily rebalancing dates the shorter window sees another universe than the pack
    (at the longer window), at every size - those (date, spec) pairs come from `_weights_for_dates` as patches, with that
    spec's own universe rows; the rest is read in the sweep's results on the device, scaled by 1 / risk_aversion."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    md, _ = synthetic.make_market_data(n_tickers=12, n_days=100, seed=20240093)
    days = md["stock_prices_df"].index
    prices = md["stock_prices_df"].copy()
    big = md["stock_market_caps_df"].loc[days[60]].idxmax()
    prices.loc[prices.index < days[30], big] = np.nan
    md = dict(md, stock_prices_df=prices)
    sizes, windows = [5, 8], [20, 40]
    specs = [_spec(5, 20, 5), _spec(5, 40, 10), _spec(8, 20, 10), _spec(8, 40, 5)]
    start, end = pd.Timestamp(days[45]), pd.Timestamp(days[80])
    trading = [pd.Timestamp(ts) for ts in days if start <= ts <= end]
    reb = pc.rebalancing_schedule(trading, "daily")
    # on the CPU, before any device call: one spec at least has served and unserved dates, and half of all pairs are served
    batch.clear_panel_cache()
    mask = batch.pack_windows_grid(reb, specs[0], sizes, windows, md)[5]
    per_spec = [mask[:, sizes.index(sp["size"]), windows.index(sp["rolling_window"])] for sp in specs]
    assert any(m.any() and not m.all() for m in per_spec)
    assert sum(int(m.sum()) for m in per_spec) * 2 >= len(reb) * len(specs)
    batch.clear_panel_cache()
    found = pc.calculate_weights_for_grid(reb, specs, md)
    tickers = batch.panels_for(md, "daily").tickers
    want = pc.replay_backtests_device(trading, reb, [(res[0], res[2], res[3], sp) for res, sp in zip(found, specs)], md,
                                      tickers=tickers)
    batch.clear_panel_cache()
    monkeypatch.setattr(_native.Device, "replay", lambda *a, **kw: pytest.fail("the host-fed replay ran"))
    sweeps = []
    real = _native.Batch.grid_sweep
    monkeypatch.setattr(_native.Batch, "grid_sweep", lambda self, *a, **kw: (sweeps.append(kw.get("want_weights")), real(self, *a, **kw))[1])
    got = pc.backtest_portfolios_grid(specs, start, end, md)
    assert sweeps == [False]                                              # one sweep, its weights never downloaded
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
