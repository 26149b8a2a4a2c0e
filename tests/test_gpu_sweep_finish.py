"""The sweep finish (-m gpu): `tp_batch_sweep_finish` / `Batch.sweep_finish` form the Greyserman and Jorion weights from the
solutions a solve sweep left on the device, `Batch.replay(REPLAY_SRC_SWEEP_FINISH, ...)` reads them where they lie.

The truth (tests/_sweep_finish_reference.py, numpy.longdouble, sequential) is fed the solutions the device itself downloaded, so
the finish kernel alone is under test.  The bound is not a measurement: per window
    |device - truth|_j <= 2^-53 (k + S + 32) amp max_j M_j,
amp = 1 (Greyserman) or the window's cancellation ratio of q (Jorion); the case builders assert the conditions it is valid under
(ratio(K12) <= 64, ratio(K22) <= 8, ratio(det) <= 2; ratio(q) <= 32) on the CPU, from the same solutions.  Everything else is
byte for byte: a window's result against itself in another batch, another chunking, another run; the replay against
`download_sweep_finish` + `Device.replay`."""
import os

import numpy as np
import pytest

from incorporating_different_sources_amd import _native, synthetic

import _sweep_finish_reference as ref
from _replay_batch_cases import _common, _yardstick
from _replay_cases import _same_bytes, _universes
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

INVALID = _native.ERR_INVALID
G = _native.FINISH_DRAWS_PER_WAVE
GAMMA = 5.0
N_R = 30


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def pc():
    from incorporating_different_sources_amd import portfolio_calculations
    return portfolio_calculations


# ---- case builders (pure functions of their arguments: the same cases on the CPU and on the device) ---------------------
def panel_of(k, W, n_r, seed):
    """W disjoint windows of n_r one-factor rows each; window w starts at row w n_r."""
    return np.concatenate([ref.one_factor_window(k, n_r, seed + 97 * w) for w in range(W)], axis=0)


def hyper_of(W, S, seed):
    pairs = [ref.draws(S, seed + 13 * w) for w in range(W)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def shift_of(eta):
    sh = np.zeros(eta.shape + (2,))
    sh[..., 0] = eta / 2
    return sh


def greyserman_batch(dev, k, W, n_r, seed, panel=None, gamma=1.0):
    b = dev.batch("jeffreys", k, n_r + 1, n_r, gamma, W, 0, _native.FLAG_NO_CENTER)
    b.upload(panel_of(k, W, n_r, seed) if panel is None else panel, start=np.arange(W, dtype=np.int64) * n_r)
    return b


def jorion_batch(dev, k, W, n_r, seed):
    b = dev.batch("jeffreys", k, n_r + 1, n_r, 1.0, W, 0, _native.FLAG_CENTER_BY_ROWS)
    b.upload(panel_of(k, W, n_r, seed), start=np.arange(W, dtype=np.int64) * n_r)
    return b


def sweep(b, shift, download=False):
    call = b.solve_sweep_tiled if b.k > _native.sweep_max_assets() else b.solve_sweep
    return call(shift=shift, rhs=np.ones((b.W, 1, b.k)), default_rhs=True, download=download)


def greyserman_finish(b, n, xi, eta, gamma=GAMMA, want_aux=False):
    W = b.W
    kappa = np.full(W, ref.greyserman_kappa(n))
    return b.sweep_finish(_native.FINISH_GREYSERMAN, np.full(W, float(n)), gamma, kappa=kappa, xi=xi, eta=eta) \
            .download_sweep_finish(want_aux=want_aux)


def check_greyserman(b, n, xi, eta, got, what):
    """`got` = (weights, status, aux) of the finish against the truth fed the device's own solutions."""
    x, xs = b.download_sweep()
    t = b.download_sweep_rhs()
    assert (xs == _native.STATUS_OK).all(), what
    weights, status, aux = got
    assert (status == _native.STATUS_OK).all(), (what, status)
    S, k = xi.shape[1], b.k
    for w in range(b.W):
        truth = ref.greyserman_truth(x[w, :, 0, :], x[w, :, 1, :], t[w], n, ref.greyserman_kappa(n), xi[w], eta[w], GAMMA)
        ref.assert_greyserman_case(truth, f"{what} w={w}")
        err, bound = float(np.abs(weights[w] - truth["weights"]).max()), ref.bound(k, S, truth["M"])
        print(f"{what} w={w}: err {err:.3e} bound {bound:.3e} ratios {truth['ratios']}")
        assert err <= bound, f"{what} w={w}: {err:.3e} > {bound:.3e}"
        if aux is not None:
            np.testing.assert_allclose(aux[w], truth["aux"], rtol=1e-9, atol=0, err_msg=what)   # (what a failure needs to see)


S_VALUES = [1, 2, G - 1, G, G + 1, 2 * G + 1]


# ---- A. Greyserman against the truth ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 143, 144, 200])
def test_greyserman_matches_truth(dev, k):
    W = 3
    with greyserman_batch(dev, k, W, N_R, 5100 + k) as b:
        for S in S_VALUES:
            xi, eta = hyper_of(W, S, 5235 + 31 * k + S)      # (seeds chosen so that the conditions of the bound hold)
            sweep(b, shift_of(eta))
            check_greyserman(b, N_R, xi, eta, greyserman_finish(b, N_R, xi, eta, want_aux=True), f"k={k} S={S}")


def test_greyserman_far_edge_k2046(dev):
    """k + R = 2048: 32 columns per lane; the ridge keeps the 12-row window positive definite."""
    k, W, S, n_r = 2046, 1, 2, 12
    with greyserman_batch(dev, k, W, n_r, 5300) as b:
        xi, eta = hyper_of(W, S, 5301)
        eta = eta + 2.0
        sweep(b, shift_of(eta))
        check_greyserman(b, n_r, xi, eta, greyserman_finish(b, n_r, xi, eta, want_aux=True), "k=2046")


def test_xi_zero_is_finite_and_beta_zero_is_flagged(dev):
    k, W, S = 10, 3, 5                                        # k < n_r: positive definite without a ridge, so eta = 0 solves
    with greyserman_batch(dev, k, W, N_R, 5400) as b:
        xi, eta = hyper_of(W, S, 5401)
        xi[1, 2] = 0.0
        sweep(b, shift_of(eta))
        clean = greyserman_finish(b, N_R, xi, eta)
        check_greyserman(b, N_R, xi, eta, clean, "xi=0")
        assert np.isfinite(clean[0]).all()
        eta[1, 2] = 0.0                                       # beta = eta / 2 + kappa xi^2 = 0
        sweep(b, shift_of(eta))
        _x, xs = b.download_sweep()
        assert (xs == _native.STATUS_OK).all()
        weights, status, _ = greyserman_finish(b, N_R, xi, eta)
        assert list(status) == [_native.STATUS_OK, _native.STATUS_NONFINITE, _native.STATUS_OK]
        assert weights[0].tobytes() == clean[0][0].tobytes() and weights[2].tobytes() == clean[0][2].tobytes()


# ---- B. Jorion against the truth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_r", [(4, 44), (63, 103), (100, 140), (143, 183), (200, 260)])
def test_jorion_matches_truth(dev, k, n_r):
    first = None
    for W in (5, 1):
        with jorion_batch(dev, k, W, n_r, 6100 + k) as b:
            sweep(b, None)
            weights, status, aux = b.sweep_finish(_native.FINISH_JORION, np.full(W, float(n_r)), GAMMA).download_sweep_finish(True)
            x, xs = b.download_sweep()
            t = b.download_sweep_rhs()
        assert (xs == _native.STATUS_OK).all() and (status == _native.STATUS_OK).all()
        for w in range(W):
            truth = ref.jorion_truth(x[w, 0, 0], x[w, 0, 1], t[w], n_r, GAMMA)
            ref.assert_jorion_case(truth, f"k={k} w={w}")
            err, bound = float(np.abs(weights[w] - truth["weights"]).max()), ref.bound(k, 1, truth["M"], amp=truth["ratio_q"])
            print(f"jorion k={k} W={W} w={w}: err {err:.3e} bound {bound:.3e} ratio(q) {truth['ratio_q']:.3g}")
            assert err <= bound
            np.testing.assert_allclose(aux[w, 0], truth["aux"], rtol=1e-9, atol=0)
        if first is None:
            first = weights[0].tobytes()
        else:
            assert weights[0].tobytes() == first              # window 0 alone and among five


# ---- C. statuses --------------------------------------------------------------------------------------------------------
def test_nan_rows_flag_their_window_only(dev):
    k, W, S = 20, 4, G + 2
    xi, eta = hyper_of(W, S, 6202)
    panel = panel_of(k, W, N_R, 6200)
    with greyserman_batch(dev, k, W, N_R, 0, panel=panel) as b:
        sweep(b, shift_of(eta))
        clean = greyserman_finish(b, N_R, xi, eta)
    assert (clean[1] == _native.STATUS_OK).all()
    bad = panel.copy()
    bad[2 * N_R + 7, 3] = np.nan
    with greyserman_batch(dev, k, W, N_R, 0, panel=bad) as b:
        sweep(b, shift_of(eta))
        _x, xs = b.download_sweep()
        weights, status, _ = greyserman_finish(b, N_R, xi, eta)
    assert xs[2, 0] != _native.STATUS_OK and status[2] == xs[2, 0]
    assert np.isnan(weights[2]).all()
    for w in (0, 1, 3):
        assert status[w] == _native.STATUS_OK and weights[w].tobytes() == clean[0][w].tobytes()


def test_one_shift_not_pd_flags_its_window(dev):
    k, W, S = 63, 3, G + 3                                    # 30 rows < 63 columns: singular without a ridge
    xi, eta = hyper_of(W, S, 6301)
    eta = eta + 0.5
    with greyserman_batch(dev, k, W, N_R, 6300) as b:
        sweep(b, shift_of(eta))
        clean = greyserman_finish(b, N_R, xi, eta)
        assert (clean[1] == _native.STATUS_OK).all()
        shift = shift_of(eta)
        shift[1, G + 1, 0] = 0.0                              # (window 1, one shift of its second group) alone
        sweep(b, shift)
        _x, xs = b.download_sweep()
        weights, status, aux = greyserman_finish(b, N_R, xi, eta, want_aux=True)
    assert xs[1, G + 1] == _native.STATUS_NOT_PD and (np.delete(xs.reshape(-1), S + G + 1) == _native.STATUS_OK).all()
    assert list(status) == [_native.STATUS_OK, _native.STATUS_NOT_PD, _native.STATUS_OK]
    assert np.isnan(weights[1]).all() and np.isnan(aux[1, G + 1]).all() and np.isfinite(aux[1, :G + 1]).all()
    assert weights[0].tobytes() == clean[0][0].tobytes() and weights[2].tobytes() == clean[0][2].tobytes()


# ---- D. determinism -----------------------------------------------------------------------------------------------------
def test_a_window_is_the_same_bits_alone_among_seven_chunked_and_again(dev):
    k, W, S = 50, 7, 2 * G + 1
    panel = panel_of(k, W, N_R, 6400)
    xi, eta = hyper_of(W, S, 6401)

    def run(windows, chunk=0):
        dev.set_option("sweep_chunk_windows", chunk)
        try:
            rows = np.concatenate([panel[w * N_R:(w + 1) * N_R] for w in windows], axis=0)
            with greyserman_batch(dev, k, len(windows), N_R, 0, panel=rows) as b:
                sweep(b, shift_of(eta[windows]))
                return greyserman_finish(b, N_R, xi[windows], eta[windows], want_aux=True)
        finally:
            dev.set_option("sweep_chunk_windows", 0)

    every = list(range(W))
    all7 = run(every)
    assert (all7[1] == _native.STATUS_OK).all()
    assert _same_bytes(run(every), all7)
    assert _same_bytes(run(every, chunk=2), all7)
    alone = run([3])
    assert alone[0][0].tobytes() == all7[0][3].tobytes() and alone[2][0].tobytes() == all7[2][3].tobytes()


# ---- E. refusals --------------------------------------------------------------------------------------------------------
def refused(call, text):
    with pytest.raises(_native.TangencyError) as e:
        call()
    assert e.value.code == INVALID and text in str(e.value), str(e.value)


def test_refusals(dev):
    k, W, S = 6, 2, 3
    xi, eta = hyper_of(W, S, 6501)
    n, kappa = np.full(W, float(N_R)), np.full(W, 3.0)
    grey = lambda b, **kw: b.sweep_finish(_native.FINISH_GREYSERMAN, n, kw.pop("gamma", GAMMA), kappa=kappa,   # noqa: E731
                                          xi=kw.pop("xi", xi), eta=kw.pop("eta", eta))
    with greyserman_batch(dev, k, W, N_R, 6500) as b:
        refused(lambda: grey(b), "no tp_batch_solve_sweep before it")
        refused(lambda: b.download_sweep_finish(), "no tp_batch_sweep_finish before it")
        b.solve_sweep(shift=shift_of(eta), default_rhs=True)                               # R = 1
        refused(lambda: grey(b), "R = 2")
        b.solve_sweep(shift=shift_of(eta), rhs=np.ones((W, 2, k)), default_rhs=False)      # R = 2 without the default
        refused(lambda: grey(b), "without the default one")
        sweep(b, shift_of(eta[:, :2]))
        refused(lambda: b.sweep_finish(_native.FINISH_JORION, n, GAMMA), "one shift per window")
        sweep(b, shift_of(eta))
        bad_eta = eta.copy()
        bad_eta[1, 1] = np.nan
        refused(lambda: grey(b, eta=bad_eta), "is not finite")
        refused(lambda: grey(b, gamma=0.0), "must be finite and not 0")
        good = grey(b).download_sweep_finish(want_aux=True)
        assert (good[1] == _native.STATUS_OK).all()
        refused(lambda: grey(b, gamma=0.0), "must be finite and not 0")                    # a refused call ...
        refused(lambda: grey(b, eta=bad_eta), "is not finite")
        assert _same_bytes(b.download_sweep_finish(want_aux=True), good)                   # ... leaves the last finish in place
        sweep(b, shift_of(eta))                                                            # a new sweep replaces the solutions
        refused(lambda: b.download_sweep_finish(), "replaced the solutions")
        rng = np.random.default_rng(6502)
        K = 2 * k + 7
        universe = dict(cols=_universes(rng, W, k, K), caps=rng.lognormal(3, 1, (W, k)), u_off=np.zeros(1, dtype=np.int64),
                        u_stride=np.full(1, k, dtype=np.int64), scaling=np.array([5.0]), cost=np.array([15.0]))
        refused(lambda: b.replay(_native.REPLAY_SRC_SWEEP_FINISH, k=np.array([k], dtype=np.int32), w_off=np.zeros(1, dtype=np.int64),
                                 w_stride=np.full(1, k, dtype=np.int64), s_off=np.zeros(1, dtype=np.int64),
                                 s_stride=np.ones(1, dtype=np.int64), **_common(rng, W, K), **universe), "replaced the solutions")
    with greyserman_batch(dev, k, W, N_R, 6500, gamma=5.0) as b:
        sweep(b, shift_of(eta))
        refused(lambda: grey(b), "gamma = 1 is expected")


# ---- F. the replay source -----------------------------------------------------------------------------------------------
def test_replay_source(dev):
    k, R, D, S = 10, 12, 60, G + 1
    rng = np.random.default_rng(6600)
    K = 2 * k + 7
    common = _common(rng, R, K, D=D)
    universe = dict(cols=_universes(rng, R, k, K), caps=rng.lognormal(3, 1, (R, k)), u_off=np.zeros(1, dtype=np.int64),
                    u_stride=np.full(1, k, dtype=np.int64), scaling=np.array([GAMMA]), cost=np.array([15.0]))
    zeros, stride = np.zeros(1, dtype=np.int64), np.full(1, k, dtype=np.int64)
    where = dict(k=np.array([k], dtype=np.int32), w_off=zeros, w_stride=stride, s_off=zeros, s_stride=np.ones(1, dtype=np.int64))
    xi, eta = hyper_of(R, S, 6601)
    panel = panel_of(k, R, N_R, 6602)
    with greyserman_batch(dev, k, R, N_R, 0, panel=panel) as b:
        sweep(b, shift_of(eta))
        weights, status, _ = greyserman_finish(b, N_R, xi, eta)
        assert (status == _native.STATUS_OK).all()
        got = b.replay(_native.REPLAY_SRC_SWEEP_FINISH, **where, **common, **universe)
        want = _yardstick(dev, common, [k], universe, weights, zeros, stride)
        assert (got[3] == 0).all() and np.isfinite(got[0][:, 1:]).all()
        assert _same_bytes(got, want)
        assert _same_bytes(b.download_sweep_finish(), (weights, status))          # the replay wrote nothing into the batch
        stats, sstatus = dev.replay_summary(np.array([0.0, 15.0]), np.zeros(D))
        assert stats.shape == (1, 2, _native.SUMMARY_STATS) and (sstatus == _native.SUMMARY_OK).all()
    bad = panel.copy()
    bad[5 * N_R + 2, 1] = np.nan                              # date 5 is flagged by the sweep, and so by the finish
    with greyserman_batch(dev, k, R, N_R, 0, panel=bad) as b:
        sweep(b, shift_of(eta))
        flagged, fstatus, _ = greyserman_finish(b, N_R, xi, eta)
        assert fstatus[5] != _native.STATUS_OK and (np.delete(fstatus, 5) == _native.STATUS_OK).all()
        got = b.replay(_native.REPLAY_SRC_SWEEP_FINISH, **where, **common, **universe)
        assert got[3][0] == _native.REPLAY_BAD_WEIGHTS and got[4][0] == common["reb_day"][5]
        patches = (np.zeros(1, dtype=np.int64), np.array([5], dtype=np.int32), weights[5][None, :].copy())
        got = b.replay(_native.REPLAY_SRC_SWEEP_FINISH, patches=patches, **where, **common, **universe)
        want = _yardstick(dev, common, [k], universe, flagged, zeros, stride, patches=patches)
        assert (got[3] == 0).all() and _same_bytes(got, want)


# ---- G. the surface -----------------------------------------------------------------------------------------------------
GREYSERMAN_RTOL = 1e-6                                       # tests/test_gpu_boundary.py


def _spec(strat, size, N, window_freq, rebal):
    return {"weighting_strategy": strat, "size": size, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": rebal,
            "rolling_window": N, "rolling_window_frequency": window_freq, "mcm_scaling": None, "display_name": strat}


def test_calculate_greyserman_portfolio_with_the_device_finish(pc, monkeypatch):
    g = np.load(os.path.join(GOLDEN, "greyserman_single.npz"))
    for k, N in ((10, 60), (33, 80), (100, 250)):
        seed = int(g[f"k{k}_n{N}_seed"])
        inp = synthetic.make_kernel_inputs(k, N, 2, seed)
        tickers = [f"A{i:04d}" for i in range(k)]
        for w in range(2):
            date, prices_df, _intraday_df, _caps_df, rf_df = synthetic.window_frames(inp, w, tickers)
            spec = _spec("greyserman", k, N, "daily", "daily")
            want = g[f"k{k}_n{N}_w{w}_weights"]
            monkeypatch.setattr(pc, "GREYSERMAN_DEVICE_FINISH", True)
            np.random.seed(seed + w)
            on = pc.calculate_greyserman_portfolio(spec, date, prices_df, rf_df)
            assert list(on.index) == tickers and on.index.name == "Stock"
            np.testing.assert_allclose(on["Weight"].to_numpy(), want, rtol=0, atol=GREYSERMAN_RTOL * np.abs(want).max())
            # fixed draws, flag on against flag off: both consume the same device solutions, each is within the bound of the truth
            # (draws of the test's own: the reference's 1000 include one whose K12 cancels past the bound's condition)
            golden = (g[f"k{k}_n{N}_w{w}_xi"], g[f"k{k}_n{N}_w{w}_eta"])
            again = pc.calculate_greyserman_portfolio(spec, date, prices_df, rf_df, draws=golden)["Weight"].to_numpy()
            assert again.tobytes() == on["Weight"].to_numpy().tobytes()
            draws = ref.draws(1000, 7000 + 10 * k + w)
            fixed_on = pc.calculate_greyserman_portfolio(spec, date, prices_df, rf_df, draws=draws)["Weight"].to_numpy()
            monkeypatch.setattr(pc, "GREYSERMAN_DEVICE_FINISH", False)
            seen = {}
            host = pc._greyserman_from_solves

            def spy(u_t, u_one, t, n, xi, eta, k_, gamma, seen=seen, host=host):
                seen.update(u_t=u_t, u_one=u_one, t=t, n=n, xi=xi, eta=eta)
                return host(u_t, u_one, t, n, xi, eta, k_, gamma)

            monkeypatch.setattr(pc, "_greyserman_from_solves", spy)
            off = pc.calculate_greyserman_portfolio(spec, date, prices_df, rf_df, draws=draws)["Weight"].to_numpy()
            monkeypatch.setattr(pc, "_greyserman_from_solves", host)
            n = float(np.asarray(seen["n"]).reshape(-1)[0])
            truth = ref.greyserman_truth(seen["u_t"][0], seen["u_one"][0], seen["t"][0], n, ref.greyserman_kappa(n),
                                         seen["xi"][0], seen["eta"][0], 5.0)
            ref.assert_greyserman_case(truth, f"k={k} w={w}")
            err, bound = float(np.abs(fixed_on - off).max()), 2 * ref.bound(k, len(draws[0]), truth["M"])
            print(f"surface k={k} w={w}: |on - off| {err:.3e}, 2 x bound {bound:.3e}")
            assert err <= bound


def _golden_backtest(pc, name, strat):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    md, _tickers = synthetic.make_market_data(n_tickers=int(g["n_tickers"]), n_days=int(g["n_days"]), seed=int(g["seed"]),
                                              rf_nan_every=int(g["rf_nan_every"]))
    days = md["stock_prices_df"].index
    spec = _spec(strat, int(g["size"]), int(g["N"]), str(g["window_freq"]), str(g["rebal"]))
    return g, md, spec, days[int(g["start_idx"])], days[-1]


def _against_weights_then_replay(pc, spec, start, end, md, res, reseed=None):
    """`_weights_for_dates` (the device finish switched on by the caller) + `replay_backtests_device`: bit for bit `res`."""
    trading = [ts for ts in md["stock_prices_df"].index if start <= ts <= end]
    reb = pc.rebalancing_schedule(trading, spec["rebalancing_frequency"])
    if reseed is not None:
        np.random.seed(reseed)
    weights, _labels, cols, caps = pc._weights_for_dates(reb, spec, md)
    want = pc.replay_backtests_device(trading, reb, [(weights, cols, caps, spec)], md)[0]
    for key in ("portfolio_simple_returns_series", "portfolio_turnover_series", "portfolio_weights_metrics_df"):
        assert res[key].to_numpy().tobytes() == want[key].to_numpy().tobytes(), key
        assert res[key].index.equals(want[key].index)


def test_backtest_portfolio_device_greyserman(pc, monkeypatch):
    g, md, spec, start, end = _golden_backtest(pc, "backtest_k10_n60_daily_greyserman", "greyserman")
    np.random.seed(int(g["np_seed"]))
    res = pc.backtest_portfolio_device(spec, start, end, md)
    tol = dict(rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(res["portfolio_simple_returns_series"].to_numpy(), g["greyserman_returns"], **tol)
    np.testing.assert_allclose(res["portfolio_turnover_series"].to_numpy(), g["greyserman_turnover"], **tol)
    np.testing.assert_allclose(res["portfolio_weights_metrics_df"].to_numpy(), g["greyserman_metrics"], equal_nan=True, **tol)
    monkeypatch.setattr(pc, "GREYSERMAN_DEVICE_FINISH", True)
    _against_weights_then_replay(pc, spec, start, end, md, res, reseed=int(g["np_seed"]))


def test_backtest_portfolio_device_jorion(pc, monkeypatch):
    g, md, spec, start, end = _golden_backtest(pc, "backtest_k10_n60_daily_jorion", "jorion")
    res = pc.backtest_portfolio_device(spec, start, end, md)
    tol = dict(rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res["portfolio_simple_returns_series"].to_numpy(), g["jorion_returns"], **tol)
    np.testing.assert_allclose(res["portfolio_turnover_series"].to_numpy(), g["jorion_turnover"], **tol)
    np.testing.assert_allclose(res["portfolio_weights_metrics_df"].to_numpy(), g["jorion_metrics"], equal_nan=True, **tol)
    monkeypatch.setattr(pc, "JORION_DEVICE_FINISH", True)
    _against_weights_then_replay(pc, spec, start, end, md, res)
