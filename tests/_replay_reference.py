"""The truth for the backtest replay: the daily loop of a backtest (mark to market, drift and renormalisation, rebalancing,
turnover over the union of the two universes with NaN counted as 0, the turnover cost, the five weight metrics) restated
plainly in numpy.longdouble - 80-bit on x86, eps 1.1e-19 against float64's 2.2e-16.  No tests in here.

It uses no project code beyond `_rf_asof` and `rebalancing_schedule`, which build inputs that both replays receive as
float64.  Everything both sides are GIVEN as float64 (returns, risk-free rates, weights, caps, `cost / 10000`, the scaling)
enters exactly; everything they COMPUTE is computed here in long double.  There is no sum check: that check is about rounding,
not about the model.

`replay_reference_arrays` works on plain arrays (what `Device.replay` receives), `replay_reference` has the argument shapes
of `portfolio_calculations._replay_backtest`.  Both return long-double arrays (returns[1:], turnover[1:], metrics)."""
import numpy as np
import pandas as pd

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not an extended-precision type on this host"

_NAN = LD("nan")


def _nansum(x):
    """Sum of the entries that are not NaN (0 for none), accumulated in long double."""
    return x[~np.isnan(x)].sum(dtype=LD)


def _nan_as_zero(x):
    return np.where(np.isnan(x), LD(0), x)


def replay_reference_arrays(S, rf_daily, reb_day, weights, cols, caps, scaling=1, cost=0):
    """`S` [D x >= K] simple returns, `rf_daily` [D], `reb_day` [R] trading-day indices (reb_day[0] == 0), `weights`, `cols`,
    `caps` [R x k], `scaling` and `cost` (basis points) scalars.  Returns (returns [D-1], turnover [R-1], metrics [R x 5])."""
    S = np.asarray(S, dtype=np.float64)
    D = S.shape[0]
    reb_day = [int(d) for d in reb_day]
    R = len(reb_day)
    weights = np.asarray(weights, dtype=np.float64).reshape(R, -1)
    cols = np.asarray(cols).reshape(R, -1)
    caps = np.asarray(caps, dtype=np.float64).reshape(R, -1)
    assert reb_day[0] == 0 and weights.shape == cols.shape == caps.shape
    cost_frac = LD(np.float64(cost) / np.float64(10000))      # formed in float64 by the kernel and by the host
    scaling = LD(np.float64(scaling))
    returns = np.full(D, _NAN, dtype=LD)
    turnover = np.full(R, _NAN, dtype=LD)
    metrics = np.full((R, 5), _NAN, dtype=LD)
    date_of = {d: j for j, d in enumerate(reb_day)}
    w = held = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for d in range(D):
            if d > 0:
                r = S[d, held].astype(LD)
                rf = LD(rf_daily[d])
                cash = 1 - _nansum(w)
                returns[d] = _nansum(r * w) + cash * rf
                cash_after = cash * (1 + rf)
                drifted = w * (1 + r)
                w = drifted / (_nansum(drifted) + cash_after)
            j = date_of.get(d)
            if j is None:
                continue
            before, before_held = w, held
            w, held = weights[j].astype(LD), cols[j]
            longs, shorts = w[w > 0], w[w < 0]
            if longs.size:
                metrics[j, 0], metrics[j, 2] = longs.max(), _nansum(longs) / longs.size
            if shorts.size:
                metrics[j, 1], metrics[j, 3] = shorts.min(), _nansum(shorts) / shorts.size
            c = caps[j].astype(LD)
            distance = np.abs(w * scaling - c / _nansum(c))
            if (~np.isnan(distance)).any():
                metrics[j, 4] = _nansum(distance) / (~np.isnan(distance)).sum()
            if before is None:
                continue
            position = np.zeros((2, S.shape[1]), dtype=LD)     # per ticker: the weight before and after, NaN as 0; a
            position[0, before_held] = _nan_as_zero(before)    # ticker outside both universes contributes |0 - 0|
            position[1, held] = _nan_as_zero(w)
            traded = np.abs(position[0] - position[1]).sum(dtype=LD)
            turnover[j] = (traded + abs(_nansum(before) - _nansum(w))) / 2
            returns[d] = returns[d] - cost_frac * turnover[j]
    return returns[1:], turnover[1:], metrics


def replay_reference(trading_dates, rebalance_dates, weights, cols, caps, tickers, portfolio_spec, market_data):
    """The argument shapes of `_replay_backtest`."""
    from incorporating_different_sources_amd.portfolio_calculations import _rf_asof
    S = market_data["stock_simple_returns_df"].reindex(index=pd.DatetimeIndex(trading_dates), columns=tickers)
    rf_daily = (_rf_asof(market_data["risk_free_rate_df"], trading_dates) + 1) ** (1 / 252) - 1
    day_of = {ts: d for d, ts in enumerate(trading_dates)}
    scaling = portfolio_spec["risk_aversion"] if portfolio_spec.get("risk_aversion") is not None else 1
    return replay_reference_arrays(S.to_numpy(dtype=np.float64), rf_daily, [day_of[ts] for ts in rebalance_dates], weights,
                                   cols, caps, scaling, portfolio_spec["turnover_cost"])
