"""Evaluation of backtests (ref: src/portfolio_evaluation.py, cited as ref:LINE): the reference's metrics table from the
records the device reduces a replay to (`_native.Device.replay_summary`, csrc/replay_summary.hip), one record of
SUMMARY_STATS doubles per (portfolio, trading cost).

`get_insolvent_date`, `adjust_returns` and `compute_excess_returns` restate the reference's helpers without its Python loops.
`summary_records_host` forms the same records in plain numpy, sequentially: the yardstick of the device's records and nothing
else - the product keeps no CPU path.  `performance_table` turns records into the rows of `performance_metrics` (ref:464-701).

The rows the reference takes from QuantStats (pinned at 0.0.62 there) are defined HERE by the formulas below; where the
reference checks a QuantStats value against a formula of its own (`CHECK`, ref:524, 541, 592, 607, 623, 655) that formula is
the definition.  Parity of Sortino, Max. DD and Daily VaR with QuantStats itself is not pinned.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

SUMMARY_STATS = 32
SUMMARY_OK, SUMMARY_NO_REPLAY, SUMMARY_NONFINITE = 0, 1, 2
# fields of a record (include/tangency_posterior.h, tp_replay_summary)
(N_OBS, ADJ_DAY, INSOLVENT_DAY, COMP, MEAN, STD, MAX_DD, BEST, WORST, SUM_WIN, N_WIN, SUM_LOSS, N_LOSS, N_PRE, MEAN_PRE, STD_PRE,
 WORST_PRE, SUM_NONZERO, N_NONZERO, ADJ_DAY_E, MEAN_E, STD_E, M2_E, M3_E, M4_E, DOWNSIDE_E, TURNOVER_SUM, TURNOVER_N) = range(28)
KEPT_WHEN_NONFINITE = (N_OBS, ADJ_DAY, INSOLVENT_DAY, ADJ_DAY_E)

METRICS = ["Cum. Return", "CAGR", "Sharpe", "Prob. Sharpe", "Sortino", "Calmar", "Max. DD", "Avg. Loss", "Avg. Return", "Avg. Win",
           "Best Day", "Worst Day", "Ann. Vol.", "Daily VaR", "Avg. Turnover"]
# None for an insolvent portfolio (ref:520-576)
NONE_WHEN_INSOLVENT = ("CAGR", "Sharpe", "Prob. Sharpe", "Sortino", "Calmar")


def _first(mask):
    hit = np.flatnonzero(mask)
    return int(hit[0]) if hit.size else -1


def get_insolvent_date(returns_series):
    """ref:27-33: the label of the first day whose compounded return is below -99 %, or None."""
    compounded = (1 + returns_series).cumprod() - 1
    i = _first((compounded < -0.99).to_numpy())
    return None if i < 0 else returns_series.index[i]


def adjust_returns(series):
    """ref:46-72 without the loop over prefixes: up to the first day whose compounded return is below -100 % the prefixes of the
    adjusted series are the prefixes of `series`, so one cumulative product finds that day.  It is set to -1 when it is the
    first day and to 0.000001 / prev_cum_return - 1 otherwise (ref:61, as written: a zero `prev_cum_return` gives inf), and
    every later day to 0."""
    adjusted = series.copy()
    compounded = (1 + series).cumprod() - 1
    i = _first((compounded < -1).to_numpy())
    if i < 0:
        return adjusted
    with np.errstate(divide="ignore"):
        adjusted.iloc[i] = -1 if i == 0 else np.float64(0.000001) / np.float64(compounded.iloc[i - 1]) - 1
    adjusted.iloc[i + 1:] = 0
    return adjusted


def _daily_rate(rate_series, index):
    """ref:706-713: the annual rate as of every date of `index` - the last quote before a gap, the next one before the first -
    as a daily rate."""
    matched = rate_series.reindex(index).ffill().bfill()
    return (matched + 1) ** (1 / 252) - 1


def compute_excess_returns(portfolio_simple_returns_series, risk_free_rate_df):
    """ref:703-718."""
    excess = portfolio_simple_returns_series - _daily_rate(risk_free_rate_df["DTB3"], portfolio_simple_returns_series.index)
    excess.name = portfolio_simple_returns_series.name
    return excess


def rf_excess_for(trading_dates, risk_free_rate_df):
    """`rf_excess` [D] as `Device.replay_summary` and `summary_records_host` take it: what `compute_excess_returns` subtracts on
    the days of a backtest's returns, trading_dates[1:]; entry 0 (never read) is NaN."""
    days = pd.DatetimeIndex(trading_dates)
    out = np.full(len(days), np.nan)
    out[1:] = _daily_rate(risk_free_rate_df["DTB3"], days[1:]).to_numpy(dtype=np.float64)
    return out


def _adjust(v):
    """`adjust_returns` on an array: (adjusted, index of the changed entry or -1)."""
    with np.errstate(all="ignore"):
        wealth = np.cumprod(1 + v)
        i = _first(wealth - 1 < -1)
        if i < 0:
            return v, -1
        out = v.copy()
        out[i] = -1.0 if i == 0 else 0.000001 / (wealth[i - 1] - 1) - 1
        out[i + 1:] = 0.0
    return out, i


def _std(v, mean):
    return np.sqrt(np.sum((v - mean) ** 2) / (v.size - 1)) if v.size >= 2 else np.nan


def summary_records_host(returns, turnover, reb_day, cost_bp, rf_excess, replay_status=None):
    """The records of `tp_replay_summary` in plain numpy - every series in double exactly as the header defines it, the products
    and sums in numpy's own sequential / pairwise order: (stats [P, C, SUMMARY_STATS], status [P, C]).  `returns` [P, D] and
    `turnover` [P, R] are a replay's at cost 0 (`Device.replay`), `reb_day` [R], `cost_bp` [C] basis points, `rf_excess` [D];
    `replay_status` [P]: the replay's statuses (None: all 0)."""
    returns = np.asarray(returns, dtype=np.float64)
    turnover = np.asarray(turnover, dtype=np.float64)
    reb = np.asarray(reb_day, dtype=np.int64)
    costs = np.asarray(cost_bp, dtype=np.float64).reshape(-1)
    rf = np.asarray(rf_excess, dtype=np.float64)
    P, D = returns.shape
    R = reb.size
    if D < 2 or turnover.shape != (P, R) or rf.shape != (D,):
        raise ValueError(f"returns [P, D >= 2], turnover [P, R] and rf_excess [D] expected, got {returns.shape}, "
                         f"{turnover.shape}, {rf.shape}")
    stats = np.zeros((P, costs.size, SUMMARY_STATS))
    status = np.zeros((P, costs.size), dtype=np.int32)
    n = D - 1
    charged = reb[1:]                                           # (date 0 has no portfolio before it: ref:1212 never runs)
    with np.errstate(all="ignore"):
        for p in range(P):
            if replay_status is not None and replay_status[p] != 0:
                stats[p, :, :28] = np.nan
                status[p] = SUMMARY_NO_REPLAY
                continue
            for c, cost in enumerate(costs):
                x = returns[p, 1:].copy()
                x[charged - 1] = returns[p, charged] - (cost / 10000.0) * turnover[p, 1:]
                e = x - rf[1:]
                a, adj_a = _adjust(x)
                b, adj_b = _adjust(e)
                wealth = np.cumprod(1 + a)
                ins = _first(wealth - 1 < -0.99)
                rec = stats[p, c]
                rec[N_OBS], rec[ADJ_DAY], rec[INSOLVENT_DAY], rec[ADJ_DAY_E] = n, adj_a + 1 if adj_a >= 0 else -1, \
                    ins + 1 if ins >= 0 else -1, adj_b + 1 if adj_b >= 0 else -1
                if not (np.isfinite(a).all() and np.isfinite(b).all()):
                    rec[[i for i in range(28) if i not in KEPT_WHEN_NONFINITE]] = np.nan
                    status[p, c] = SUMMARY_NONFINITE
                    continue
                pre = a if ins < 0 else a[:ins]
                rec[COMP] = wealth[-1] - 1
                rec[MEAN] = np.sum(a) / n
                rec[STD] = _std(a, rec[MEAN])
                rec[MAX_DD] = np.min(wealth / np.maximum.accumulate(wealth) - 1)
                rec[BEST], rec[WORST] = a.max(), a.min()
                rec[SUM_WIN], rec[N_WIN] = np.sum(a[a > 0]), np.count_nonzero(a > 0)
                rec[SUM_LOSS], rec[N_LOSS] = np.sum(a[a < 0]), np.count_nonzero(a < 0)
                rec[N_PRE] = pre.size
                rec[MEAN_PRE] = np.sum(pre) / pre.size if pre.size else np.nan
                rec[STD_PRE] = _std(pre, rec[MEAN_PRE])
                rec[WORST_PRE] = pre.min() if pre.size else np.nan
                moved = np.abs(a) > 1e-7
                rec[SUM_NONZERO], rec[N_NONZERO] = np.sum(a[moved]), np.count_nonzero(moved)
                rec[MEAN_E] = np.sum(b) / n
                centred = b - rec[MEAN_E]
                rec[STD_E] = _std(b, rec[MEAN_E])
                rec[M2_E], rec[M3_E], rec[M4_E] = (np.sum(centred ** q) / n for q in (2, 3, 4))
                rec[DOWNSIDE_E] = np.sum(b[b < 0] ** 2) / n
                traded = turnover[p, 1:] if ins < 0 else turnover[p, 1:][charged <= ins + 1]
                rec[TURNOVER_SUM], rec[TURNOVER_N] = np.sum(traded), traded.size
    return stats, status


def benchmark_sharpe(benchmark_excess):
    """ref:86-88: mean / std (ddof = 1) of the benchmark's daily excess returns, not annualised."""
    v = np.asarray(benchmark_excess, dtype=np.float64)
    return np.mean(v) / np.std(v, ddof=1)


def performance_table(stats, status, trading_dates, names, cost_bp, benchmark_excess=None):
    """The rows of `performance_metrics` (ref:464-701) from summary records: a DataFrame indexed by (name, cost) with one column
    per metric (`METRICS`).  `stats` [P, C, SUMMARY_STATS] and `status` [P, C] are `Device.replay_summary`'s (or
    `summary_records_host`'s), `trading_dates` the D days of the backtest - its returns are dated trading_dates[1:] -, `names`
    [P], `cost_bp` [C].  `benchmark_excess`: the benchmark's daily excess returns for Prob. Sharpe (ref:78-120, ref:555: the
    S&P 500's); without them that column is NaN.

        CAGR = (COMP + 1) ** (1 / ((last - first).days / 365)) - 1 (ref:524) ;  Sharpe = MEAN_E / STD_E sqrt(252) (ref:541)
        Sortino = MEAN_E / sqrt(DOWNSIDE_E) sqrt(252) ;  Calmar = CAGR / |MAX_DD| ;  Ann. Vol. = STD_PRE sqrt(252) (ref:655, 660)
        Daily VaR = norm.ppf(0.05, MEAN_PRE, STD_PRE) ;  Avg. Turnover = TURNOVER_SUM / TURNOVER_N (ref:694-696)
        Avg. Loss = SUM_LOSS / N_LOSS, Avg. Win = SUM_WIN / N_WIN, Avg. Return = MEAN, or SUM_NONZERO / N_NONZERO when insolvent
        (ref:612) ;  Worst Day = WORST_PRE (ref:644)
        Prob. Sharpe = norm.cdf((sr - benchmark sr) / sqrt((1 - skew sr + (kurt - 1) / 4 sr^2) / (n - 1))), sr = MEAN_E / STD_E,
        skew = M3_E / M2_E^1.5, kurt = M4_E / M2_E^2 (scipy's biased estimators)

    An insolvent portfolio (INSOLVENT_DAY >= 0) has None in CAGR, Sharpe, Prob. Sharpe, Sortino and Calmar (ref:520-576); those
    columns have dtype object.  A record whose status is not SUMMARY_OK gives a row of NaN."""
    from scipy.stats import norm

    stats = np.asarray(stats, dtype=np.float64)
    status = np.asarray(status)
    costs = np.asarray(cost_bp, dtype=np.float64).reshape(-1)
    names = list(names)
    if stats.shape != (len(names), costs.size, SUMMARY_STATS) or status.shape != stats.shape[:2]:
        raise ValueError(f"stats [{len(names)}, {costs.size}, {SUMMARY_STATS}] and status [{len(names)}, {costs.size}] expected, "
                         f"got {stats.shape} and {status.shape}")
    days = pd.DatetimeIndex(trading_dates)
    years = (days[-1] - days[1]).days / 365
    bench = np.nan if benchmark_excess is None else benchmark_sharpe(benchmark_excess)
    s = np.where((status == SUMMARY_OK)[..., None], stats, np.nan).reshape(-1, SUMMARY_STATS).T
    with np.errstate(all="ignore"):
        cagr = (s[COMP] + 1) ** (1 / years) - 1
        sr = s[MEAN_E] / s[STD_E]
        skewness, kurt = s[M3_E] / s[M2_E] ** 1.5, s[M4_E] / s[M2_E] ** 2
        sr_sigma = np.sqrt((1 - skewness * sr + (kurt - 1) / 4 * sr ** 2) / (s[N_OBS] - 1))
        solvent = s[INSOLVENT_DAY] < 0
        cols = {
            "Cum. Return": s[COMP],
            "CAGR": cagr,
            "Sharpe": sr * 252 ** 0.5,
            "Prob. Sharpe": norm.cdf((sr - bench) / sr_sigma),
            "Sortino": s[MEAN_E] / np.sqrt(s[DOWNSIDE_E]) * 252 ** 0.5,
            "Calmar": cagr / np.abs(s[MAX_DD]),
            "Max. DD": s[MAX_DD],
            "Avg. Loss": s[SUM_LOSS] / s[N_LOSS],
            "Avg. Return": np.where(solvent, s[MEAN], s[SUM_NONZERO] / s[N_NONZERO]),
            "Avg. Win": s[SUM_WIN] / s[N_WIN],
            "Best Day": s[BEST],
            "Worst Day": s[WORST_PRE],
            "Ann. Vol.": s[STD_PRE] * 252 ** 0.5,
            "Daily VaR": norm.ppf(0.05, s[MEAN_PRE], s[STD_PRE]),
            "Avg. Turnover": s[TURNOVER_SUM] / s[TURNOVER_N],
        }
    index = pd.MultiIndex.from_product([names, costs.tolist()], names=["name", "turnover_cost"])
    table = pd.DataFrame({m: cols[m] for m in METRICS}, index=index)
    insolvent = s[INSOLVENT_DAY] >= 0
    for m in NONE_WHEN_INSOLVENT:
        col = table[m].astype(object)
        col[insolvent] = None
        table[m] = col
    return table
