"""Backtest engine and Bayesian weight estimators with the reference's call surface
(`/root/reference/src/portfolio_calculations.py`, cited below as ref:LINE), MI355X-native underneath.

What is different from the reference is WHERE the arithmetic runs and HOW OFTEN the host touches
pandas:

* every rebalancing date of a backtest is known up front (the schedule depends only on the date list,
  ref:1166-1176), so `backtest_portfolio` extracts all windows first, sends them to the GPU in ONE
  batched call (`_native.posterior_batch` -> `libtangency.so`, include/tangency_posterior.h) and then
  replays the cheap sequential P&L loop (ref:1127-1219) with the weights already in hand;
* the per-window statistics (T, t, S0, c, S1, w1, q1, nu: ref:163-608) never exist on the host: the
  fused HIP kernel produces the weights directly.  The same-named helper functions below exist for
  API compatibility and run a one-window batch on the device.

There is no CPU fallback for the estimators: without `libtangency.so` and a gfx950 GPU they raise.
The passive weightings (vw / ew, ref:661-701) are host-side, as they are inputs (prior weights w0 and
the comparison portfolio), not part of the accelerated path.  Jorion's Bayes-Stein portfolio (ref:851-895)
reuses the device's scatter + Cholesky solve with two right-hand sides, and so does the Greyserman
hierarchical prior (ref:897-938), one ridge-shifted window per hyper-parameter draw.  Shrinkage and
Black-Litterman (ref:703-817: pypfopt, not in the tree) are outside the scope of this build and raise
NotImplementedError - unless the caller registers the reference's own two functions with
`register_strategy` (a caller who has pypfopt), which the dispatch then calls date by date.
"""
from __future__ import annotations

import logging
import os
from datetime import timedelta

import numpy as np
import pandas as pd

try:  # importable both as a package module and as a top-level `portfolio_calculations` (main.py style)
    from . import _native, batch, portfolio_evaluation, portfolio_specs, shard
except ImportError:  # pragma: no cover - top-level import with the package directory on sys.path
    import _native  # type: ignore
    import batch  # type: ignore
    import portfolio_evaluation  # type: ignore
    import portfolio_specs  # type: ignore
    import shard  # type: ignore

logging_level = os.environ.get("LOGGING_LEVEL", logging.INFO)
logging.basicConfig(level=logging_level)
logger = logging.getLogger(__name__)

# The reference's CHECK flag (ref:30): with it on, every helper re-derives its result a second way on the host and
# raises the reference's ValueError when the two disagree (ref:81-86 w'Sw, ref:185-202 T against the sum of outer
# products, ref:225-242 t against the sum of rows, ref:321-330 the intraday scatter against Y'Y, ref:420-428 the two
# algebraic forms of c) - here the first way is the DEVICE's matrix, read back with tp_batch_download_matrix.  The
# checks are O(n k^2) Python / numpy work per window, so the flag defaults to off (the reference ships it on).
CHECK = False

_CONJUGATE = ("conjugate_hf_vix_vw", "conjugate_hf_vix_ew", "conjugate_hf_epu_vw", "conjugate_hf_epu_ew")
_OUT_OF_SCOPE = ("shrinkage", "black_litterman")
_RESAMPLE_RULE = {"weekly": "W", "monthly": "ME"}


# ======================================================================================================
# small frequency tables (ref:116-134, 299-308, 628-637)
def get_window_annualization_factor(portfolio_spec):
    return {"daily": 252, "weekly": 52, "monthly": 12}[portfolio_spec["rolling_window_frequency"]]


def get_window_trading_days(portfolio_spec):
    per_period = {"daily": 1, "weekly": 5, "monthly": 22}[portfolio_spec["rolling_window_frequency"]]
    return portfolio_spec["rolling_window"] * per_period


def _calendar_days_of(frequency):
    try:
        return {"daily": 1, "weekly": 7, "monthly": 31}[frequency]
    except KeyError:
        logger.error("Unknown rolling window frequency.")
        raise RuntimeError("Unknown rolling window frequency.")


def _resample_last(df, frequency):
    """ref:149-156 / ref:102-109: last observation per calendar week / month ('daily' = unchanged)."""
    if frequency == "daily":
        return df
    if frequency not in _RESAMPLE_RULE:
        return df
    try:
        return df.resample(_RESAMPLE_RULE[frequency]).last()
    except ValueError:  # pandas < 2.2 spells month-end 'M'
        return df.resample("M" if frequency == "monthly" else "W").last()


def _require_last_date(df, trading_date_ts):
    if trading_date_ts != df.index[-1]:
        logger.error(f"trading_date_ts {trading_date_ts} is not the last date in the DataFrame.")
        raise ValueError(f"trading_date_ts {trading_date_ts} must be the last date in the DataFrame.")


# ======================================================================================================
# window preparation on the host (ref:31-62, 136-161): label logic, no O(n k^2) work
def adjust_stock_prices_window(portfolio_spec, trading_date_ts, k_stock_prices_df):
    """Last `rolling_window` (resampled) price rows ending at the trading date (ref:136-161)."""
    k_stock_prices_df = k_stock_prices_df.sort_index()
    _require_last_date(k_stock_prices_df, trading_date_ts)
    window = _resample_last(k_stock_prices_df, portfolio_spec["rolling_window_frequency"])
    return window.iloc[-portfolio_spec["rolling_window"]:]


def calculate_excess_log_returns_from_prices(portfolio_spec, stock_prices_df, risk_free_rate_df):
    """log(P_t/P_{t-1}) minus the risk-free rate scaled to the mean calendar gap of the window's
    dates; rows with any NaN are dropped (ref:31-62)."""
    log_returns = np.log(stock_prices_df / stock_prices_df.shift(1))
    rf_rows = _rf_adjustment_for(stock_prices_df.index, risk_free_rate_df)
    excess = log_returns - rf_rows[:, None]
    return excess.dropna()


def _rf_adjustment_for(index, risk_free_rate_df):
    """Per-row risk-free adjustment for a window's date labels (ref:40-54): annual simple rate ->
    per-period via the MEAN calendar-day gap / 365, forward-filled on labels (NaN values stay NaN)."""
    gaps = index.to_series().diff().dt.days.dropna()
    mean_gap = gaps.mean()
    assert gaps.max() <= mean_gap + 4, "Unexpected large gap between return dates."
    adjusted = (1 + risk_free_rate_df) ** (mean_gap / 365) - 1
    adjusted.index = risk_free_rate_df.index
    return adjusted.reindex(index, method="ffill").to_numpy().reshape(len(index), -1)[:, 0]


def _daily_window_arrays(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """Host packing of one window for the device: raw log-returns (n_r x k), the per-row risk-free
    adjustment (subtracted on the device, ref:57) and the asset labels."""
    window = adjust_stock_prices_window(portfolio_spec, trading_date_ts, k_stock_prices_df)
    values = window.to_numpy(dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_returns = np.log(values[1:] / values[:-1])
    rf_rows = _rf_adjustment_for(window.index, risk_free_rate_df)[1:]
    keep = ~np.isnan(log_returns).any(axis=1) & ~np.isnan(rf_rows)     # dropna (ref:60)
    return np.ascontiguousarray(log_returns[keep]), np.ascontiguousarray(rf_rows[keep]), list(window.columns)


def _host_excess_returns(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """X (n_r x k) on the host, for the CHECK identities only (the device subtracts the risk-free rate itself)."""
    log_returns, rf_rows, _ = _daily_window_arrays(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
    return log_returns - rf_rows[:, None]


def _intraday_window_returns(portfolio_spec, trading_date_ts, k_stock_intraday_prices_df):
    """Intraday log-returns of the last period (ref:299-314): bars in (date+1d-Delta, date+1d]."""
    span = _calendar_days_of(portfolio_spec["rolling_window_frequency"])
    lo = trading_date_ts - pd.Timedelta(days=span) + pd.Timedelta(days=1)
    hi = trading_date_ts + pd.Timedelta(days=1)
    idx = k_stock_intraday_prices_df.index
    bars = k_stock_intraday_prices_df[(idx > lo) & (idx <= hi)]
    values = bars.to_numpy(dtype=np.float64)
    if len(values) < 2:
        return np.empty((0, values.shape[1] if values.ndim == 2 else 0)), list(bars.columns)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_returns = np.log(values[1:] / values[:-1])
    keep = ~np.isnan(log_returns).any(axis=1)
    return np.ascontiguousarray(log_returns[keep]), list(bars.columns)


# ======================================================================================================
# prior hyper-parameters that are host scalars (ref:90-114, 247-282)
def calculate_average_mcm_window(portfolio_spec, trading_date_ts, mcm_prices_df):
    mcm_prices_df = mcm_prices_df.sort_index()
    _require_last_date(mcm_prices_df, trading_date_ts)
    window = _resample_last(mcm_prices_df, portfolio_spec["rolling_window_frequency"])
    return window.iloc[-portfolio_spec["rolling_window"]:].mean().item()


def calculate_conjugate_prior_n(portfolio_spec, trading_date_ts, mcm_prices_df):
    """n0 = N * max(cur/avg, avg/cur) * mcm_scaling (ref:247-267, Appendix B-Q5)."""
    average = calculate_average_mcm_window(portfolio_spec, trading_date_ts, mcm_prices_df)
    current = mcm_prices_df.loc[trading_date_ts].item()
    fraction = current / average if current > average else average / current
    return portfolio_spec["rolling_window"] * fraction * portfolio_spec["mcm_scaling"]


def calculate_conjugate_posterior_n(portfolio_spec, trading_date_ts, mcm_prices_df, conjugate_prior_n=None):
    if conjugate_prior_n is None:
        conjugate_prior_n = calculate_conjugate_prior_n(portfolio_spec, trading_date_ts, mcm_prices_df)
    return conjugate_prior_n + portfolio_spec["rolling_window"]


# ======================================================================================================
# passive weightings: host side (prior weights / comparison portfolio), ref:661-701
def calculate_equally_weighted_portfolio(portfolio_spec, k_stock_prices_df):
    n = portfolio_spec["size"]
    out = pd.DataFrame({"Weight": [1 / n] * n}, index=k_stock_prices_df.columns)
    out.index.name = "Stock"
    return out


def calculate_value_weighted_portfolio(portfolio_spec, trading_date_ts, k_stock_market_caps_df):
    caps = k_stock_market_caps_df.iloc[-1].sort_values(ascending=False)
    assert k_stock_market_caps_df.index[-1] == trading_date_ts, "The last index date does not match the trading date."
    out = pd.DataFrame(caps / caps.sum())
    out.index.name = "Stock"
    out.columns = ["Weight"]
    return out


def calculate_conjugate_prior_w(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                                mcm_prices_df):
    strategy = portfolio_spec["weighting_strategy"]
    if "vw" in strategy:
        return calculate_value_weighted_portfolio(portfolio_spec, trading_date_ts, k_stock_market_caps_df)
    if "ew" in strategy:
        return calculate_equally_weighted_portfolio(portfolio_spec, k_stock_prices_df)
    logger.error("Unknown conjugate portfolio prior weights.")
    raise ValueError("Unknown conjugate portfolio prior weights.")


def calculate_portfolio_variance(portfolio_weights_df, covariance_matrix_df):
    """w'Sw with label alignment (ref:64-88).  API-compatibility helper: the fused kernel forms q0
    and q1 itself and never calls this."""
    w = portfolio_weights_df.sort_index()
    S = covariance_matrix_df.loc[w.index, w.index].to_numpy()
    v = w["Weight"].to_numpy()
    variance = float(v @ (S @ v))
    if CHECK:  # ref:81-86: the label-aligned pandas product of the unsorted frames gives the same number
        check = portfolio_weights_df["Weight"].T.dot(covariance_matrix_df.dot(portfolio_weights_df["Weight"]))
        if not np.isclose(variance, check, atol=1e-4):
            raise ValueError("Portfolio variance is not consistent.")
    return variance


# ======================================================================================================
# one window on the device
class _WindowOnDevice:
    """One window packed from the reference-style frames and resident on the GPU: the estimator
    helpers below pull whichever quantity they are named after out of it."""

    def __init__(self, portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df,
                 k_stock_market_caps_df=None, k_stock_intraday_prices_df=None, mcm_prices_df=None,
                 conjugate_prior_n=None, conjugate_prior_w_df=None, strategy=None):
        self.spec = portfolio_spec
        X, rf_rows, labels = _daily_window_arrays(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
        self.labels = labels
        k = len(labels)
        self.k = k
        N = portfolio_spec["rolling_window"]
        conj = (strategy or portfolio_spec["weighting_strategy"]) != "jeffreys"
        gamma = portfolio_spec.get("risk_aversion") or 1.0
        kw = dict(panel=X, start=np.zeros(1, np.int64), rf_adj=rf_rows[None, :])
        m = 0
        self.n0 = None
        self.w0_df = None
        if conj:
            Y, hf_labels = _intraday_window_returns(portfolio_spec, trading_date_ts, k_stock_intraday_prices_df)
            Y = Y[:, [hf_labels.index(s) for s in labels]] if hf_labels != labels else Y
            m = Y.shape[0]
            if conjugate_prior_n is None:
                conjugate_prior_n = calculate_conjugate_prior_n(portfolio_spec, trading_date_ts, mcm_prices_df)
            if conjugate_prior_w_df is None:
                conjugate_prior_w_df = calculate_conjugate_prior_w(portfolio_spec, trading_date_ts, k_stock_prices_df,
                                                                   k_stock_market_caps_df, mcm_prices_df)
            self.n0 = float(conjugate_prior_n)
            self.w0_df = conjugate_prior_w_df
            w0 = conjugate_prior_w_df["Weight"].reindex(labels).to_numpy(dtype=np.float64)
            kw.update(hf_panel=Y, hf_start=np.zeros(1, np.int64), w0=w0[None, :], n0=np.array([self.n0]))
        if portfolio_spec["size"] != k:
            raise ValueError(f"portfolio_spec['size']={portfolio_spec['size']} but the frame has {k} assets")
        dev = _native.default_device()
        self.batch = _native.Batch(dev, "conjugate" if conj else "jeffreys", k, N, max(X.shape[0], 1), gamma, 1, m)
        self.batch.upload(**kw)

    def weights(self):
        w, status, aux = self.batch.run().download()
        _raise_on_status(status)
        return w[0], aux[0]

    def matrix(self, what):
        M, rhs = self.batch.download_matrix(0, what)
        return M, rhs

    def frame(self, M):
        return pd.DataFrame(M, index=self.labels, columns=self.labels)

    def close(self):
        self.batch.close()


def _raise_on_status(status):
    status = np.asarray(status)
    if (status == _native.STATUS_NONFINITE).any() or (status == _native.STATUS_NOT_PD).any():
        # ref:492-494 raises on NaN weights; a non-positive-definite S1 is reported the same way
        # instead of returning the finite garbage an LU inverse would give (Appendix B-Q8)
        logger.error("conjugate_posterior_w_df contains NaN values.")
        raise ValueError("conjugate_posterior_w_df contains NaN values.")


def _weights_frame(values, labels):
    out = pd.DataFrame({"Weight": np.asarray(values, dtype=np.float64)}, index=pd.Index(labels))
    return out


def calculate_canonical_statistics_T(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """T = X'X (ref:163-204) - fp64 MFMA Gram on the device."""
    win = _WindowOnDevice(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df, strategy="jeffreys")
    try:
        T, _ = win.matrix("gram")
        if CHECK:  # ref:185-202: T against the sum of the rows' outer products
            X = _host_excess_returns(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
            T_check = np.zeros_like(T)
            for xi in X:
                T_check += np.outer(xi, xi)
            if not np.isclose(T, T_check, rtol=1e-4, atol=1e-4).all():
                raise ValueError("Canonical statistics T is not consistent.")
        return win.frame(T)
    finally:
        win.close()


def calculate_canonical_statistics_t(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """t = X'1 (ref:206-245), returned as a one-column frame like `Series.to_frame()`."""
    win = _WindowOnDevice(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df, strategy="jeffreys")
    try:
        _, t = win.matrix("gram")
        if CHECK:  # ref:225-242: t against the sum of the rows
            X = _host_excess_returns(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
            t_check = np.zeros_like(t)
            for xi in X:
                t_check += xi
            if not np.isclose(t, t_check, rtol=1e-4, atol=1e-4).all():
                raise ValueError("Canonical statistics t is not consistent.")
        return pd.DataFrame({0: t}, index=pd.Index(win.labels))
    finally:
        win.close()


def calculate_conjugate_prior_S(portfolio_spec, trading_date_ts, k_stock_intraday_prices_df, mcm_prices_df,
                                conjugate_prior_n=None):
    """S0 = n0 * cov(Y) * len(Y) (ref:285-333)."""
    if conjugate_prior_n is None:
        conjugate_prior_n = calculate_conjugate_prior_n(portfolio_spec, trading_date_ts, mcm_prices_df)
    Y, labels = _intraday_window_returns(portfolio_spec, trading_date_ts, k_stock_intraday_prices_df)
    k = len(labels)
    dev = _native.default_device()
    # a one-row dummy daily window: only the prior phase of the kernel is read back
    b = _native.Batch(dev, "conjugate", k, portfolio_spec["rolling_window"], 1, 1.0, 1, Y.shape[0])
    try:
        b.upload(panel=np.zeros((1, k)), start=np.zeros(1, np.int64), hf_panel=Y, hf_start=np.zeros(1, np.int64),
                 w0=np.full((1, k), 1.0 / k), n0=np.array([float(conjugate_prior_n)]))
        S0, _ = b.download_matrix(0, "prior")
    finally:
        b.close()
    if CHECK:  # ref:321-330: cov(Y) * len(Y) against the uncentred Y'Y (rtol = atol = 1e-3, as in the reference)
        if not np.isclose(S0 / conjugate_prior_n, Y.T @ Y, rtol=1e-3, atol=1e-3).all():
            raise ValueError("Realized covariance matrix is not consistent.")
    return pd.DataFrame(S0, index=labels, columns=labels)


def calculate_conjugate_posterior_S(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_intraday_prices_df,
                                    mcm_prices_df, risk_free_rate_df, conjugate_prior_S_df=None):
    """S1 = S0 + T (ref:335-358)."""
    if conjugate_prior_S_df is not None:
        T = calculate_canonical_statistics_T(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
        return conjugate_prior_S_df + T
    spec = dict(portfolio_spec)
    win = _WindowOnDevice(spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df,
                          k_stock_intraday_prices_df=k_stock_intraday_prices_df, mcm_prices_df=mcm_prices_df,
                          conjugate_prior_w_df=calculate_equally_weighted_portfolio(spec, k_stock_prices_df),
                          strategy="conjugate")
    try:
        S1, _ = win.matrix("posterior")
        return win.frame(S1)
    finally:
        win.close()


def _conjugate_window(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                      k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df, conjugate_prior_n=None,
                      conjugate_prior_w_df=None):
    return _WindowOnDevice(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df,
                           k_stock_market_caps_df=k_stock_market_caps_df,
                           k_stock_intraday_prices_df=k_stock_intraday_prices_df, mcm_prices_df=mcm_prices_df,
                           conjugate_prior_n=conjugate_prior_n, conjugate_prior_w_df=conjugate_prior_w_df,
                           strategy="conjugate")


def calculate_conjugate_c(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                          k_stock_intraday_prices_df, mcm_prices_df, conjugate_prior_n=None,
                          conjugate_prior_S_df=None, conjugate_prior_w_df=None):
    """c = 2 n0 / (a + sqrt(a^2 + 4 n0 w0'S0 w0)), a = n0 + size + 2 (ref:382-430)."""
    if conjugate_prior_n is None:
        conjugate_prior_n = calculate_conjugate_prior_n(portfolio_spec, trading_date_ts, mcm_prices_df)
    if conjugate_prior_w_df is None:
        conjugate_prior_w_df = calculate_conjugate_prior_w(portfolio_spec, trading_date_ts, k_stock_prices_df,
                                                           k_stock_market_caps_df, mcm_prices_df)
    if conjugate_prior_S_df is not None:
        q0 = calculate_portfolio_variance(conjugate_prior_w_df, conjugate_prior_S_df)
        a = conjugate_prior_n + portfolio_spec["size"] + 2
        return (2 * conjugate_prior_n) / (a + (a ** 2 + 4 * conjugate_prior_n * q0) ** (1 / 2))
    Y, labels = _intraday_window_returns(portfolio_spec, trading_date_ts, k_stock_intraday_prices_df)
    k = len(labels)
    dev = _native.default_device()
    b = _native.Batch(dev, "conjugate", portfolio_spec["size"], portfolio_spec["rolling_window"], 1, 1.0, 1, Y.shape[0])
    try:
        w0 = conjugate_prior_w_df["Weight"].reindex(labels).to_numpy(dtype=np.float64)
        b.upload(panel=np.zeros((1, k)), start=np.zeros(1, np.int64), hf_panel=Y, hf_start=np.zeros(1, np.int64),
                 w0=w0[None, :], n0=np.array([float(conjugate_prior_n)]))
        _, _, aux = b.run().download()
    finally:
        b.close()
    c = float(aux[0, 2])
    if CHECK:  # ref:420-428: the two algebraic forms of c agree
        q0 = float(aux[0, 3])
        a = conjugate_prior_n + portfolio_spec["size"] + 2
        c_check = (-a + (a ** 2 + 4 * conjugate_prior_n * q0) ** (1 / 2)) / (2 * q0)
        if not np.isclose(c, c_check, atol=1e-3):
            raise ValueError("Portfolio c is not consistent.")
    return c


def calculate_conjugate_posterior_w(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                                    k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df, conjugate_c=None,
                                    conjugate_prior_w_df=None, conjugate_prior_S_df=None,
                                    conjugate_posterior_S_df=None):
    """w1 = S1^-1 (c S0 w0 + t) (ref:432-496) - Cholesky solve on the device, no explicit inverse."""
    win = _conjugate_window(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                            k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df,
                            conjugate_prior_w_df=conjugate_prior_w_df)
    try:
        weights, aux = win.weights()
        n1, q1 = aux[1], aux[4]
        gamma = portfolio_spec.get("risk_aversion") or 1.0
        w1 = weights * gamma * (n1 - q1) / (n1 + portfolio_spec["size"] + 2)     # undo ref:572-575, 836
        return _weights_frame(w1, win.labels)
    finally:
        win.close()


def calculate_mean_conjugate_posterior_nu(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                                          k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df,
                                          conjugate_c=None, conjugate_prior_n=None, conjugate_posterior_n=None,
                                          conjugate_prior_S_df=None, conjugate_posterior_S_df=None,
                                          conjugate_prior_w_df=None, conjugate_posterior_w_df=None):
    """nu = (n1 + size + 2) w1 / (n1 - w1'S1 w1) (ref:499-577): the posterior MEAN of the weights."""
    win = _conjugate_window(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                            k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df,
                            conjugate_prior_n=conjugate_prior_n, conjugate_prior_w_df=conjugate_prior_w_df)
    try:
        weights, _ = win.weights()
        gamma = portfolio_spec.get("risk_aversion") or 1.0
        return _weights_frame(weights * gamma, win.labels)
    finally:
        win.close()


def calculate_mean_jeffreys_posterior_nu(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """nu = (T - t t'/N)^-1 t (ref:580-608)."""
    win = _WindowOnDevice(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df, strategy="jeffreys")
    try:
        weights, _ = win.weights()
        gamma = portfolio_spec.get("risk_aversion") or 1.0
        return _weights_frame(weights * gamma, win.labels)
    finally:
        win.close()


def calculate_conjugate_hf_mcm_portfolio(portfolio_spec, trading_date_ts, k_stock_market_caps_df, k_stock_prices_df,
                                         k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df):
    """weights = nu / risk_aversion (ref:819-836)."""
    win = _conjugate_window(portfolio_spec, trading_date_ts, k_stock_prices_df, k_stock_market_caps_df,
                            k_stock_intraday_prices_df, mcm_prices_df, risk_free_rate_df)
    try:
        weights, _ = win.weights()
        return _weights_frame(weights, win.labels)
    finally:
        win.close()


def calculate_jeffreys_portfolio(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """weights = nu / risk_aversion (ref:838-849)."""
    win = _WindowOnDevice(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df, strategy="jeffreys")
    try:
        weights, _ = win.weights()
        return _weights_frame(weights, win.labels)
    finally:
        win.close()


# Strategies of the reference's dispatch (ref:999-1011) that this build does not compute (pypfopt 1.5.5 is an un-vendored
# dependency: parity unpinned) can be supplied by the caller: name -> function with the REFERENCE's signature,
#   shrinkage        f(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)              ref:703-706
#   black_litterman  f(portfolio_spec, trading_date_ts, k_stock_market_caps_df, k_stock_prices_df,
#                      risk_free_rate_df)                                                                  ref:759-763
# returning the reference's frame (index 'Stock', column 'Weight').
_EXTERNAL_STRATEGIES = {}


def register_strategy(name, fn):
    """Let the unchanged spec loop of src/main.py:48 finish: `register_strategy("shrinkage",
    reference_module.calculate_shrinkage_portfolio)` (likewise "black_litterman") makes `calculate_portfolio_weights`
    / `backtest_portfolio` call `fn` per rebalancing date with the frames the reference's dispatch passes
    (ref:999-1011).  `fn=None` removes the registration (the strategy raises NotImplementedError again)."""
    if name not in _OUT_OF_SCOPE:
        raise ValueError(f"register_strategy: only {_OUT_OF_SCOPE} can be supplied from outside, not {name!r}")
    if fn is None:
        _EXTERNAL_STRATEGIES.pop(name, None)
    elif not callable(fn):
        raise TypeError("register_strategy: fn must be callable")
    else:
        _EXTERNAL_STRATEGIES[name] = fn


def _not_in_scope(name):
    strategy = name[len("calculate_"):-len("_portfolio")]

    def f(*args, **kwargs):
        fn = _EXTERNAL_STRATEGIES.get(strategy)
        if fn is not None:
            return fn(*args, **kwargs)
        raise NotImplementedError(
            f"{name} is outside the scope of this build (SURVEY.md section 2: C9-C12); only the conjugate and "
            "Jeffreys posteriors and the passive weightings are provided.  A caller who has pypfopt can supply the "
            f"reference's function: portfolio_calculations.register_strategy({strategy!r}, fn).")
    f.__name__ = name
    return f


calculate_shrinkage_portfolio = _not_in_scope("calculate_shrinkage_portfolio")
calculate_black_litterman_portfolio = _not_in_scope("calculate_black_litterman_portfolio")


def _external_weights_for_dates(trading_dates, portfolio_spec, market_data):
    """A registered out-of-scope strategy, date by date, with the frames the reference's dispatch slices (ref:953-988,
    999-1011); returns what `_weights_for_dates` returns."""
    strategy = portfolio_spec["weighting_strategy"]
    fn = _EXTERNAL_STRATEGIES[strategy]
    members_of = _members_provider(market_data)
    cols, labels, caps = batch.pack_universes(list(trading_dates), portfolio_spec, market_data, members_of=members_of)
    rf = market_data["risk_free_rate_df"]
    weights = np.full(caps.shape, np.nan)
    for i, ts in enumerate(trading_dates):
        uni = _Universe(ts, portfolio_spec, market_data)
        if strategy == "shrinkage":
            frame = fn(portfolio_spec, ts, uni.prices, rf)
        else:
            frame = fn(portfolio_spec, ts, uni.caps, uni.prices, rf)
        col = frame["Weight"] if "Weight" in getattr(frame, "columns", ()) else frame.iloc[:, 0]
        w = col.reindex(labels[i])
        if w.isna().any():
            raise ValueError(f"{strategy}: the registered function returned no weight for {list(w.index[w.isna()])} at {ts}")
        weights[i] = w.to_numpy(dtype=np.float64)
    return weights, labels, cols, caps


def _jorion_from_solves(x_t, x_one, t, T, N, gamma):
    """Jorion's Bayes-Stein weights (ref:869-893) from two device solves with the centred scatter
    J = (T-1) V_hat:  x_t = J^-1 t (t = X'1 = T mu_hat) and x_one = J^-1 1.  V_bar = T/(T-N-2) V_hat, so
    V_bar^-1 = kappa J^-1 with kappa = (T-N-2)(T-1)/T; V_PJ is V_bar scaled plus a multiple of 11', whose
    inverse follows from V_bar^-1 1 by Sherman-Morrison instead of the reference's second LU inverse.
    Vectorised over windows: x_t, x_one, t are [W x N], T is [W]."""
    T = np.asarray(T, dtype=np.float64)[:, None]
    kappa = (T - N - 2) * (T - 1) / T
    mu = t / T
    a = kappa * x_t / T                    # V_bar^-1 mu_hat
    b = kappa * x_one                      # V_bar^-1 1
    s_bb = b.sum(axis=1, keepdims=True)
    s_ab = a.sum(axis=1, keepdims=True)
    s_aa = (mu * a).sum(axis=1, keepdims=True)
    mu_g = s_ab / s_bb                                                   # ref:882
    q = s_aa - 2 * mu_g * s_ab + mu_g ** 2 * s_bb                        # d' V_bar^-1 d
    lam = (N + 2) / q                                                    # ref:885
    v = (N + 2) / ((N + 2) + T * q)                                      # ref:887
    alpha = 1 + 1 / (T + lam)                                            # ref:888: V_PJ = alpha V_bar + beta 11'
    beta = lam / (T * (T + 1 + lam)) / s_bb
    g = (1 - v) * a + v * mu_g * b                                       # V_bar^-1 mu_PJ (ref:889)
    sol = g / alpha - (beta / alpha ** 2) * b * g.sum(axis=1, keepdims=True) / (1 + (beta / alpha) * s_bb)
    return sol / gamma                                                   # ref:893


def _finish_sweep(b, k, shift):
    """Queues on the uploaded batch `b` the solve sweep `Batch.sweep_finish` reads - the shifts `shift` ([W x S x 2], None: one
    unshifted solve), the right-hand sides [default, 1] - and leaves its solutions on the device.  Returns `b`."""
    sweep = b.solve_sweep_tiled if k > _native.sweep_max_assets() else b.solve_sweep
    sweep(shift=shift, rhs=np.ones((b.W, 1, k)), default_rhs=True, download=False)
    return b


# True: `_jorion_batch` takes ONE solve sweep (S = 1, R = 2) and finishes on the device (`Batch.sweep_finish`), so that the
# weights exist there (`backtest_portfolio_device`).  Off: the sweep loses to the two launches at large W.
JORION_DEVICE_FINISH = False


def _jorion_batch(kw, gamma, k, N):
    """Two launches over the same resident batch: right-hand side t (default) and right-hand side 1.  (One solve sweep
    with S = 1, R = 2 gives the same pair from one Gram pass, but measured slower at this shape: DESIGN.md section 4e.)
    With JORION_DEVICE_FINISH set: that one sweep, its solutions left on the device, and `Batch.sweep_finish(FINISH_JORION)`
    - the Sherman-Morrison algebra of `_jorion_from_solves` in a kernel; [W x k] weights and statuses come down.  It loses to
    the two launches on the device at large W (section 4e) and exists so that Jorion has a device-resident result."""
    dev = _native.default_device()
    W = len(kw["n_rows"])
    b = _native.Batch(dev, "jeffreys", k, N, kw["n_r"], 1.0, W, 0, flags=_native.FLAG_CENTER_BY_ROWS)
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        if JORION_DEVICE_FINISH:
            _finish_sweep(b, k, None).sweep_finish(_native.FINISH_JORION, np.asarray(kw["n_rows"], dtype=np.float64), gamma)
            weights, status, _ = b.download_sweep_finish()
            _raise_on_status(status)
            return weights
        b.keep_rhs()                                       # the first run also leaves t = X'1 (ref:222)
        x_t, status, _ = b.run().download(want_aux=False)
        _raise_on_status(status)
        t = b.download_rhs()
        b.keep_rhs(False)
        b.set_rhs(np.ones((W, k)))
        x_one, status, _ = b.run().download(want_aux=False)
        _raise_on_status(status)
    finally:
        b.close()
    return _jorion_from_solves(x_t, x_one, t, kw["n_rows"], k, gamma)


def calculate_jorion_portfolio(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df):
    """Jorion hyper-parameter portfolio (ref:851-895): the two SPD solves run on the device."""
    X, rf_rows, labels = _daily_window_arrays(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
    k = len(labels)
    kw = dict(panel=X, start=np.zeros(1, np.int64), n_r=X.shape[0], n_rows=np.array([X.shape[0]], np.int32),
              rf_adj=rf_rows[None, :])
    w = _jorion_batch(kw, portfolio_spec["risk_aversion"], k, portfolio_spec["rolling_window"])
    return pd.DataFrame({"Weight": w[0]}, index=pd.Index(labels, name="Stock"))


# ------------------------------------------------------------------------------------------------------
# Greyserman et al. hierarchical prior (ref:897-938): a Monte-Carlo mean over hyper-parameter draws, every
# draw one SPD system D_h x = a_h of the window's size - a batched-Cholesky workload for the device.
GREYSERMAN_DRAWS = 1000            # ref:925
_GREYSERMAN_DATES_PER_LAUNCH = 32  # dates x draws windows per device batch (index arrays are repeated per draw)


def _greyserman_draws(count):
    """(xi_b, eta_b) in the reference's order from numpy's global generator (ref:926-927), so that
    `numpy.random.seed` reproduces the reference's weights.  scipy's `gamma.rvs(a=1, scale=10)` is
    `standard_gamma(1) * 10` on that same generator."""
    xi = np.empty(count)
    eta = np.empty(count)
    for i in range(count):
        xi[i] = np.random.uniform(-1000, 1000)
        eta[i] = np.random.standard_gamma(1.0) * 10
    return xi, eta


def _greyserman_from_solves(u_t, u_one, t, n, xi, eta, k, gamma):
    """Mean over draws of the weights of ref:928-931 from two device solves per draw with the ridge matrix
    B_b = T + (eta_b/2) I:  u_t = B_b^-1 t and u_one = B_b^-1 1  (T = X'X is (n-1) S + n xbar xbar' of ref:929).

    With g = n + kappa, beta = eta_b/2 + kappa xi_b^2 and a_h = (t + kappa xi_b 1)/g the scale matrix of ref:929
    is D_h = B_b + beta 1 1' - g a_h a_h' = B_b + U C U' with U = [1, t].  Woodbury over that rank-two term,
    K = C^-1 + U' B_b^-1 U, collapses (C^-1 [kappa xi_b, 1]'/g = -e_2) to
        D_h^-1 a_h = (K12 u_one - K11 u_t) / det K,
        K11 = 1/beta + 1'u_one,  K12 = 1'u_t - kappa xi_b/beta,  K22 = t'u_t - n - kappa eta_b/(2 beta),
    in which no two large terms cancel (det K is a sum of two negative terms) - unlike the LU inverse of
    D_h itself, whose condition number reaches 1e10.  Shapes: u_t, u_one [W x B x k]; t [W x k]; n [W];
    xi, eta [W x B]."""
    n = np.asarray(n, dtype=np.float64)[:, None]
    kappa = np.array([round(0.1 * v) for v in n[:, 0]], dtype=np.float64)[:, None]       # ref:920
    beta = eta / 2 + kappa * xi ** 2
    K11 = 1 / beta + u_one.sum(axis=2)
    K12 = u_t.sum(axis=2) - kappa * xi / beta
    K22 = (u_t * t[:, None, :]).sum(axis=2) - n - kappa * eta / (2 * beta)
    det = K11 * K22 - K12 ** 2
    x = (K12 / det)[:, :, None] * u_one - (K11 / det)[:, :, None] * u_t                  # D_h^-1 a_h
    nu_h = k                                                                             # ref:921
    scale = 1 / gamma * (nu_h + n + 1) * (1 - 1 / (nu_h + n - k))                        # ref:931
    return (scale[:, :, None] * x).mean(axis=1)


def _greyserman_from_spectrum(lam, V, t, n, xi, eta, k, gamma):
    """`_greyserman_from_solves` from ONE eigendecomposition T = V diag(lam) V' per window instead of the solves: every ridge
    matrix B_b = T + (eta_b/2) I has the eigenvectors of T, so with t^ = V't, o^ = V'1 and r_bj = 1 / (lam_j + eta_b/2)
        u_one = V (r_b o^),  u_t = V (r_b t^),  1'u_one = sum_j r_bj o^_j^2,  1'u_t = sum_j r_bj o^_j t^_j,  t'u_t = sum_j r_bj t^_j^2,
    the rank-two algebra is that of `_greyserman_from_solves`, and the mean over the draws is taken in the eigenbasis: one
    product with V per window.  The numpy mirror of `Batch.spectral_greyserman` (same algebra, numpy's orders of summation).
    Shapes: lam [W x k]; V [W x k x k] with V[w, :, j] the eigenvector of lam[w, j]; t [W x k]; n [W]; xi, eta [W x B]."""
    lam, V, t = np.asarray(lam, dtype=np.float64), np.asarray(V, dtype=np.float64), np.asarray(t, dtype=np.float64)
    xi, eta = np.asarray(xi, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)[:, None]
    kappa = np.array([round(0.1 * v) for v in n[:, 0]], dtype=np.float64)[:, None]       # ref:920
    that = np.einsum("wij,wi->wj", V, t)[:, None, :]
    ohat = V.sum(axis=1)[:, None, :]
    r = 1 / (lam[:, None, :] + (eta / 2)[:, :, None])
    uo, ut = r * ohat, r * that
    beta = eta / 2 + kappa * xi ** 2
    K11 = 1 / beta + (uo * ohat).sum(axis=2)
    K12 = (uo * that).sum(axis=2) - kappa * xi / beta
    K22 = (ut * that).sum(axis=2) - n - kappa * eta / (2 * beta)
    det = K11 * K22 - K12 ** 2
    x = (K12 / det)[:, :, None] * uo - (K11 / det)[:, :, None] * ut                      # V' D_h^-1 a_h
    scale = 1 / gamma * (k + n + 1) * (1 - 1 / n)                                        # ref:931 with nu_h = k
    return np.einsum("wij,wj->wi", V, (scale[:, :, None] * x).mean(axis=1))


_GREYSERMAN_SWEEP_BYTES = 1 << 30   # solutions of one sweep (dates x draws x 2 x k doubles, on the device and on the host)
# Sizes above `_native.sweep_max_assets()`: True takes one window per date and one tiled solve sweep
# (`Batch.solve_sweep_tiled`, S = draws, R = 2) instead of the replicated batch.  Off until the two have been timed
# against each other on the device.
GREYSERMAN_TILED_SWEEP = False
# True: the sweeps of `_greyserman_batch` leave their solutions on the device and `Batch.sweep_finish` forms the rank-two
# algebra and the mean over draws there - [W x k] weights come down instead of W x draws x 2 x k solutions.  Off until
# tools/time_sweep_finish.py has been run on the device.
GREYSERMAN_DEVICE_FINISH = False
# True: up to `sweep_max_assets()` `_greyserman_batch` takes ONE batch over all dates and `Batch.spectral_greyserman` - one
# eigendecomposition per date instead of one factorisation per draw, no solutions buffer and so no grouping of the dates.
# Off whatever tools/time_spectral.py measures: opt-in.
GREYSERMAN_SPECTRAL = False


def _raise_on_spectral_status(status):
    """`_raise_on_status`, and the eigensolver's own refusal."""
    _raise_on_status(status)
    if (np.asarray(status) == _native.STATUS_NO_CONVERGENCE).any():
        raise RuntimeError("greyserman: the eigensolver of the spectral sweep did not converge for a date")


def _greyserman_kappa(n_rows):
    """kappa_h = round(0.1 n) of ref:920, Python's rounding, as `_greyserman_from_solves` forms it."""
    return np.array([round(0.1 * v) for v in np.asarray(n_rows, dtype=np.float64)], dtype=np.float64)


def _greyserman_batch(kw, gamma, k, N, draws=None):
    """All dates of `kw` (the `batch.pack_windows` layout): one window per date and one solve sweep over its
    GREYSERMAN_DRAWS ridge shifts d = eta_b/2 with the right-hand sides [t, 1] (`Batch.solve_sweep`) - one Gram product
    per date.  A sweep holds dates x draws x 2 x k solutions on the device and on the host, so the dates go through in
    groups of at most _GREYSERMAN_SWEEP_BYTES of solutions (1,342 dates at k = 50, 469 at k = 143, with 1000 draws); a
    date's result does not depend on the grouping.  Above `sweep_max_assets()`: GREYSERMAN_DRAWS repeated windows per
    date, two launches per 32 dates - or, with GREYSERMAN_TILED_SWEEP set, the same loop with `Batch.solve_sweep_tiled`.
    With GREYSERMAN_DEVICE_FINISH set the solutions of a group stay on the device (they still exist there, so the grouping
    stays), `Batch.sweep_finish` forms the group's weights and [dates x k] of them come down with the statuses.
    With GREYSERMAN_SPECTRAL set, up to `sweep_max_assets()`: one batch over all dates and `Batch.spectral_greyserman`."""
    n_rows = np.asarray(kw["n_rows"])
    W = len(n_rows)
    xi, eta = _greyserman_hyper(W, draws)
    tiled = k > _native.sweep_max_assets()
    if tiled and not GREYSERMAN_TILED_SWEEP:
        return _greyserman_batch_repeated(kw, gamma, k, N, xi, eta)
    dev = _native.default_device()
    if GREYSERMAN_SPECTRAL and not tiled:                 # no solutions on the device: every date in one batch
        b = _native.Batch(dev, "jeffreys", k, N, kw["n_r"], 1.0, W, 0, flags=_native.FLAG_NO_CENTER)
        try:
            b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
            b.spectral_greyserman(n_rows.astype(np.float64), gamma, _greyserman_kappa(n_rows), xi, eta)
            weights, status, _ = b.download_spectral()
        finally:
            b.close()
        _raise_on_spectral_status(status)
        return weights
    B = eta.shape[1]
    per_window = ("start", "row_idx", "n_rows", "col_idx", "rf_adj")
    group = max(1, _GREYSERMAN_SWEEP_BYTES // (B * 2 * k * 8))
    out = np.empty((W, k))
    for lo in range(0, W, group):
        hi = min(W, lo + group)
        sub = {key: (np.asarray(val)[lo:hi] if key in per_window and val is not None else val)
               for key, val in kw.items() if key not in ("n_r", "m")}
        shift = np.zeros((hi - lo, B, 2))
        shift[:, :, 0] = eta[lo:hi] / 2                                                  # eta_b S_h = eta_b/2 (I + 11')
        b = _native.Batch(dev, "jeffreys", k, N, kw["n_r"], 1.0, hi - lo, 0, flags=_native.FLAG_NO_CENTER)
        try:
            b.upload(**sub)
            if GREYSERMAN_DEVICE_FINISH:
                _finish_sweep(b, k, shift).sweep_finish(_native.FINISH_GREYSERMAN, n_rows[lo:hi].astype(np.float64), gamma,
                                                        kappa=_greyserman_kappa(n_rows[lo:hi]), xi=xi[lo:hi], eta=eta[lo:hi])
                out[lo:hi], status, _ = b.download_sweep_finish()
                _raise_on_status(status)
                continue
            u, status = (b.solve_sweep_tiled if tiled else b.solve_sweep)(shift=shift, rhs=np.ones((hi - lo, 1, k)),
                                                                          default_rhs=True)
            _raise_on_status(status.reshape(-1))
            t = b.download_sweep_rhs()                     # the Gram pass also leaves t = X'1 (ref:222)
        finally:
            b.close()
        out[lo:hi] = _greyserman_from_solves(u[:, :, 0, :], u[:, :, 1, :], t, n_rows[lo:hi], xi[lo:hi], eta[lo:hi], k, gamma)
    return out


def _greyserman_hyper(W, draws):
    """(xi, eta) [W x B]: drawn date-major, as the reference's day loop draws, or the caller's fixed `draws`."""
    B = GREYSERMAN_DRAWS if draws is None else np.asarray(draws[0]).shape[-1]
    if draws is None:
        pairs = [_greyserman_draws(B) for _ in range(W)]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    return (np.broadcast_to(np.asarray(draws[0], dtype=np.float64), (W, B)),
            np.broadcast_to(np.asarray(draws[1], dtype=np.float64), (W, B)))


def _greyserman_batch_repeated(kw, gamma, k, N, xi, eta):
    """The path above `sweep_max_assets()`: every date's index arrays repeated once per draw."""
    dev = _native.default_device()
    n_rows = np.asarray(kw["n_rows"])
    W, B = eta.shape
    per_window = ("start", "row_idx", "n_rows", "col_idx", "rf_adj")
    out = np.empty((W, k))
    for lo in range(0, W, _GREYSERMAN_DATES_PER_LAUNCH):
        hi = min(W, lo + _GREYSERMAN_DATES_PER_LAUNCH)
        sub = {key: (np.repeat(np.asarray(val)[lo:hi], B, axis=0) if key in per_window and val is not None else val)
               for key, val in kw.items() if key not in ("n_r", "m")}
        Wb = (hi - lo) * B
        shift = np.zeros((Wb, 2))
        shift[:, 0] = eta[lo:hi].reshape(-1) / 2                                         # eta_b S_h = eta_b/2 (I + 11')
        b = _native.Batch(dev, "jeffreys", k, N, kw["n_r"], 1.0, Wb, 0, flags=_native.FLAG_NO_CENTER)
        try:
            b.set_shift(shift)
            b.upload(**sub)
            b.keep_rhs()                                   # the first run also leaves t = X'1 (ref:222)
            u_t, status, _ = b.run().download(want_aux=False)
            _raise_on_status(status)
            t = b.download_rhs()
            b.keep_rhs(False)
            b.set_rhs(np.ones((Wb, k)))
            u_one, status, _ = b.run().download(want_aux=False)
            _raise_on_status(status)
        finally:
            b.close()
        out[lo:hi] = _greyserman_from_solves(u_t.reshape(hi - lo, B, k), u_one.reshape(hi - lo, B, k),
                                             t.reshape(hi - lo, B, k)[:, 0, :], n_rows[lo:hi], xi[lo:hi], eta[lo:hi],
                                             k, gamma)
    return out


def calculate_greyserman_portfolio(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df, draws=None):
    """Greyserman portfolio (ref:897-938): 2 x 1000 ridge solves on the device, rank-two algebra on the host.
    `draws=(xi, eta)` replaces the random hyper-parameter draws (testing)."""
    X, rf_rows, labels = _daily_window_arrays(portfolio_spec, trading_date_ts, k_stock_prices_df, risk_free_rate_df)
    k = len(labels)
    kw = dict(panel=X, start=np.zeros(1, np.int64), n_r=X.shape[0], n_rows=np.array([X.shape[0]], np.int32),
              rf_adj=rf_rows[None, :])
    w = _greyserman_batch(kw, portfolio_spec["risk_aversion"], k, portfolio_spec["rolling_window"], draws=draws)
    return pd.DataFrame({"Weight": w[0]}, index=pd.Index(labels, name="Stock"))


# ======================================================================================================
# universe selection and dispatch (ref:611-658, 941-1052): host, reproduced not accelerated
def _index_constituents(trading_date_ts, market_data, stock_prices_df):
    """S&P-500 membership at the date.  The reference asks its data layer (ref:619 ->
    data_handling.extract_unique_tickers); here `market_data["index_constituents"]` may be a callable
    `f(date) -> list`, else the reference's `data_handling` module is used when importable, else every
    column counts as a member (synthetic panels)."""
    provider = market_data.get("index_constituents") if isinstance(market_data, dict) else None
    if callable(provider):
        return list(provider(trading_date_ts))
    try:
        import data_handling  # the reference's data layer, if the caller has it on sys.path
        return list(data_handling.extract_unique_tickers(trading_date_ts, trading_date_ts))
    except Exception:
        return list(stock_prices_df.columns)


def get_k_largest_stocks_market_caps(stock_market_caps_df, stock_prices_df, stock_intraday_prices_df,
                                     trading_date_ts, portfolio_size, rolling_window_days, rolling_window_frequency,
                                     tickers_list=None):
    """The `portfolio_size` largest caps among stocks with a complete price window and intraday data
    (ref:611-658).  Column-vectorised; same eligibility rules and the same nlargest ordering."""
    if tickers_list is None:
        tickers_list = _index_constituents(trading_date_ts, {}, stock_prices_df)
    span = _calendar_days_of(rolling_window_frequency)
    members = set(tickers_list)
    cols = [c for c in stock_prices_df.columns
            if c in members and c in stock_market_caps_df.columns and c in stock_intraday_prices_df.columns]
    present = [t for t in tickers_list if t in stock_market_caps_df.columns]
    logger.info(f"Fraction of tickers missing from stock_market_caps_df: "
                f"{(len(tickers_list) - len(present)) / max(len(tickers_list), 1):.2%}")
    recent = stock_prices_df.loc[:trading_date_ts, cols].tail(rolling_window_days)
    full_window = recent.notna().all(axis=0)
    bars = stock_intraday_prices_df.loc[(trading_date_ts - timedelta(days=span)):(trading_date_ts + timedelta(days=1)), cols]
    has_bars = bars.notna().any(axis=0)
    eligible = [c for c in cols if full_window[c] and has_bars[c]]
    if trading_date_ts not in stock_market_caps_df.index:
        logger.error(f"The trading date {trading_date_ts} does not exist in the market capitalizations data.")
        raise ValueError(f"The trading date {trading_date_ts} does not exist in the market capitalizations data.")
    return stock_market_caps_df.loc[trading_date_ts, eligible].dropna().nlargest(portfolio_size)


class _Universe:
    """Everything `calculate_portfolio_weights` slices out of `market_data` for one date (ref:953-988)."""

    def __init__(self, trading_date_ts, portfolio_spec, market_data):
        prices = market_data["stock_prices_df"]
        caps = market_data["stock_market_caps_df"]
        intraday = market_data["stock_intraday_prices_df"]
        tickers = _index_constituents(trading_date_ts, market_data, prices)
        # ref:960 passes the REBALANCING frequency where the callee expects the window frequency (Q7)
        top = get_k_largest_stocks_market_caps(caps, prices, intraday, trading_date_ts, portfolio_spec["size"],
                                               get_window_trading_days(portfolio_spec),
                                               portfolio_spec["rebalancing_frequency"], tickers_list=tickers)
        self.top = top
        self.caps = caps[top.index.intersection(caps.columns)].loc[:trading_date_ts]
        self.prices = prices[top.index.intersection(prices.columns)].loc[:trading_date_ts]
        end_of_day = pd.Timestamp(trading_date_ts).replace(hour=23, minute=59, second=59)
        hf = intraday[top.index.intersection(intraday.columns)]
        self.intraday = hf.loc[hf.index <= end_of_day]
        if self.prices.tail(get_window_trading_days(portfolio_spec)).isna().any().any():
            logger.error("Found NA values in the filtered stock prices.")
            raise ValueError("The filtered stock prices contain NA values.")


def _mcm_frame(portfolio_spec, trading_date_ts, market_data):
    key = "vix_prices_df" if "_vix_" in portfolio_spec["weighting_strategy"] else "epu_prices_df"
    frame = market_data[key]
    return frame.loc[frame.index <= trading_date_ts]


def _pack_window(trading_date_ts, portfolio_spec, market_data):
    """Host packing of one rebalancing date for the batched device call."""
    uni = _Universe(trading_date_ts, portfolio_spec, market_data)
    strategy = portfolio_spec["weighting_strategy"]
    rf = market_data["risk_free_rate_df"]
    X, rf_rows, labels = _daily_window_arrays(portfolio_spec, trading_date_ts, uni.prices, rf)
    item = dict(labels=labels, X=X, rf=rf_rows)
    if strategy in _CONJUGATE:
        mcm = _mcm_frame(portfolio_spec, trading_date_ts, market_data)
        Y, hf_labels = _intraday_window_returns(portfolio_spec, trading_date_ts, uni.intraday)
        if hf_labels != labels:
            Y = Y[:, [hf_labels.index(s) for s in labels]]
        w0_df = calculate_conjugate_prior_w(portfolio_spec, trading_date_ts, uni.prices, uni.caps, mcm)
        item.update(Y=Y, n0=float(calculate_conjugate_prior_n(portfolio_spec, trading_date_ts, mcm)),
                    w0=w0_df["Weight"].reindex(labels).to_numpy(dtype=np.float64))
    return item


# windows below which one GPU is used even when sharding is on (a launch per device has a fixed cost)
SHARD_MIN_WINDOWS = int(os.environ.get("TP_SHARD_MIN_WINDOWS", "2048"))
# The one-process-all-GPUs route is OPT-IN: `TP_SHARD=1` in the environment at import, or `use_device_group(group)`.
# It has never run on more than one physical GPU (this build's boxes have one; the driver's multi-GPU bench uses one
# PROCESS per GPU, bench.py), so a backtest on a multi-GPU node stays on one device unless asked - ADVICE r2.
_shard_group = None
_shard_opt_in = os.environ.get("TP_SHARD", "") not in ("", "0")


def use_device_group(group=True):
    """Shard the batched solves of `backtest_portfolio` over the devices of `group` (a `_native.DeviceGroup`; True:
    every visible GPU, `_native.default_group()`; None / False: back to one device)."""
    global _shard_group, _shard_opt_in
    if group is None or group is False:
        _shard_group, _shard_opt_in = None, False
    elif group is True:
        _shard_group, _shard_opt_in = None, True
    else:
        _shard_group, _shard_opt_in = group, True


def _device_posterior_batch(strategy, k, N, gamma, kw):
    """The batched device call behind every estimator: one device by default; with sharding opted in (`TP_SHARD=1` /
    `use_device_group`), several visible GPUs and enough windows, the windows shard over the group inside this one
    process (`shard.run_sharded`: contiguous shards, one grouped RCCL gather to device 0; the reference's driver is a
    single process, src/main.py:26)."""
    n_windows = len(kw["n_rows"]) if kw.get("n_rows") is not None else len(kw["start"])
    if _shard_opt_in and n_windows >= SHARD_MIN_WINDOWS:
        group = _shard_group if _shard_group is not None else (_native.default_group() if _native.device_count() > 1 else None)
        if group is not None and group.world > 1:
            return shard.run_sharded(group, strategy, k, N, gamma, kw, want_aux=True)
    return _native.posterior_batch(strategy, k, N, gamma, **kw)


def _dates_key(trading_dates):
    return tuple(pd.Timestamp(ts).value for ts in trading_dates)


def _spec_cache_key(portfolio_spec):
    return tuple(portfolio_spec.get(name) for name in ("weighting_strategy", "size", "risk_aversion", "rebalancing_frequency",
                                                        "rolling_window", "rolling_window_frequency", "mcm_scaling"))


def _cache_slot(portfolio_spec, trading_dates, market_data):
    """(cache dict, key, MCM frame) of a conjugate spec's weights.  The cache lives on the panels object, so it dies
    with the price / caps / intraday / risk-free frames it was computed from; the VIX / EPU frame is part of the key
    and is kept alive by the entry (its `id` cannot be recycled while the entry exists)."""
    frame = market_data["vix_prices_df" if "_vix_" in portfolio_spec["weighting_strategy"] else "epu_prices_df"]
    cache = batch.panels_for(market_data, portfolio_spec["rolling_window_frequency"]).weights_cache
    # the universe also depends on who answers "members of the index at this date": the caller's provider is part of
    # the key and is kept alive by the entry, like the frame
    provider = market_data.get("index_constituents") if isinstance(market_data, dict) else None
    provider = provider if callable(provider) else None
    return cache, (_spec_cache_key(portfolio_spec), _dates_key(trading_dates), id(frame), id(provider)), (frame, provider)


def _weights_for_dates(trading_dates, portfolio_spec, market_data):
    """(weights [W x k], labels, column indices [W x k], market caps [W x k]) for MANY rebalancing dates: one
    host pass (`batch.pack_windows`) and, for the estimators, one device batch."""
    strategy = portfolio_spec["weighting_strategy"]
    if strategy in _OUT_OF_SCOPE:
        if strategy in _EXTERNAL_STRATEGIES:
            return _external_weights_for_dates(trading_dates, portfolio_spec, market_data)
        _not_in_scope(f"calculate_{strategy}_portfolio")()
    if strategy not in _CONJUGATE and strategy not in ("jeffreys", "jorion", "greyserman", "vw", "ew"):
        logger.error("Unknown weights spec.")
        raise ValueError("Unknown weights spec.")
    members_of = _members_provider(market_data)
    k, N, gamma = portfolio_spec["size"], portfolio_spec["rolling_window"], portfolio_spec.get("risk_aversion")
    if strategy in ("vw", "ew"):
        # passive strategies: universe selection only (ref:990-997 reads neither returns nor the risk-free rate)
        cols, labels, caps = batch.pack_universes(list(trading_dates), portfolio_spec, market_data, members_of=members_of)
        if strategy == "vw":
            weights = caps / caps.sum(axis=1, keepdims=True)             # ref:692-695 (already cap-descending)
        else:
            weights = np.full(caps.shape, 1 / k)                         # ref:670-672
        return weights, labels, cols, caps
    if strategy in _CONJUGATE:
        cache, key, owners = _cache_slot(portfolio_spec, trading_dates, market_data)
        hit = cache.get(key)
        if hit is not None and hit[1][0] is owners[0] and hit[1][1] is owners[1]:      # filled by a cross-spec batch
            return hit[0]
    kw, labels, caps = batch.pack_windows(list(trading_dates), portfolio_spec, market_data, members_of=members_of,
                                          return_caps=True)
    cols = kw["col_idx"]
    if strategy == "jorion":
        kw.pop("start", None)
        weights = _jorion_batch(kw, gamma, k, N)
    elif strategy == "greyserman":
        weights = _greyserman_batch(kw, gamma, k, N)
    else:
        conj = strategy in _CONJUGATE
        weights, status, aux = _device_posterior_batch("conjugate" if conj else "jeffreys", k, N, gamma, kw)
        _raise_on_status(status)
    return weights, labels, cols, caps


def _batch_family(portfolio_spec):
    """Conjugate specs with equal (size, window, frequencies) see the same windows: only w0 / n0 / gamma differ."""
    return tuple(portfolio_spec.get(name) for name in ("size", "rebalancing_frequency", "rolling_window", "rolling_window_frequency"))


def _prior_sweep_weights(k, N, gamma, kw, n0, w0, tiled=False):
    """One upload of the windows in `kw` and ONE prior sweep (`Batch.prior_sweep`; `tiled`: `Batch.prior_sweep_tiled`):
    weights [W x P x k], status [W x P] for the priors n0 [W x P], w0 [W x P x k]."""
    dev = _native.default_device()
    W = len(kw["n_rows"]) if kw.get("n_rows") is not None else len(kw["start"])
    upload = {key: val for key, val in kw.items() if key not in ("n_r", "m")}
    b = _native.Batch(dev, "conjugate", k, N, kw["n_r"], gamma, W, kw.get("m") or 0)
    try:
        b.upload(**upload)
        weights, status, _ = (b.prior_sweep_tiled if tiled else b.prior_sweep)(n0, w0, want_aux=False)
    finally:
        b.close()
    return weights, status


def calculate_weights_for_specs(trading_dates, portfolio_specs_list, market_data, share_grams=False):
    """Weights of SEVERAL conjugate specs of one grid for the same dates with ONE host pack, ONE upload of the
    panels and ONE device batch of len(specs) x len(dates) windows ("vectorised over days
    and over specs"): the specs share the windows (rows, columns, risk-free adjustment, intraday rows) and differ in
    the prior only - w0 (vw / ew, ref:361-380), n0 (VIX / EPU, mcm_scaling, ref:247-267) and gamma.  Returns one
    (weights, labels, cols, caps) per spec, bit-identical to `_weights_for_dates` spec by spec (windows are
    independent), and remembers them for the `backtest_portfolio` calls that follow.

    `share_grams=True`: the windows are uploaded ONCE (no replica per spec) and one prior sweep (`Batch.prior_sweep`) forms
    every window's two Grams once and solves the len(specs) priors from them; same results within the solve's rounding,
    same cache slots.  Sizes above `_native.sweep_max_assets()` run the replicated batch.

    `share_grams="any"`: as `True`, and sizes above `_native.sweep_max_assets()` take the large-k form of the sweep
    (`Batch.prior_sweep_tiled`) instead of the replicated batch.  Its intraday scatter is centred through the raw moments
    (DESIGN.md section 4h): for return panels the results agree with the replicated batch within the solve's rounding."""
    specs = list(portfolio_specs_list)
    if not specs:
        return []
    if any(sp["weighting_strategy"] not in _CONJUGATE for sp in specs) or len({_batch_family(sp) for sp in specs}) != 1:
        raise ValueError("calculate_weights_for_specs: conjugate specs of equal size, window and frequencies expected")
    trading_dates = list(trading_dates)
    members_of = _members_provider(market_data)
    first = specs[0]
    kw, labels, caps = batch.pack_windows(trading_dates, first, market_data, members_of=members_of, return_caps=True)
    n_dates, n_specs = len(trading_dates), len(specs)
    k, N = first["size"], first["rolling_window"]
    gammas = [sp["risk_aversion"] for sp in specs]
    same_gamma = all(g == gammas[0] for g in gammas)
    priors = [(kw["w0"], kw["n0"])] + [batch.prior_inputs(trading_dates, sp, market_data, caps) for sp in specs[1:]]
    small = bool(share_grams) and k <= _native.sweep_max_assets()
    if small or share_grams == "any":
        weights, status = _prior_sweep_weights(k, N, gammas[0] if same_gamma else 1.0, kw,
                                               np.stack([p[1] for p in priors], axis=1), np.stack([p[0] for p in priors], axis=1),
                                               tiled=not small)
        _raise_on_status(status.reshape(-1))
        weights = np.ascontiguousarray(weights.transpose(1, 0, 2)).reshape(n_specs * n_dates, k)
    else:
        weights = _replicated_weights(kw, priors, n_specs, k, N, gammas[0] if same_gamma else 1.0)
    return _fill_spec_cache(specs, trading_dates, market_data, weights, n_dates, same_gamma, labels, kw["col_idx"], caps)


# `calculate_weights_for_sizes` with a largest size above `_native.sweep_max_assets()`: True packs every requested size once at
# the largest and takes one tiled size sweep (`Batch.size_sweep_tiled`) - the sizes below that bound are then prefixes of the
# same sweep - instead of one `_weights_for_dates` per size above it.  Off: DESIGN.md section 4k holds the timings a later
# change decides the default from.
SIZE_SWEEP_TILED = False


def _size_family(portfolio_spec):
    """Specs with equal (window, frequencies) see the same dates' rows; `size` picks a prefix of the cap-ordered universe."""
    return tuple(portfolio_spec.get(name) for name in ("rebalancing_frequency", "rolling_window", "rolling_window_frequency"))


def calculate_weights_for_sizes(trading_dates, portfolio_specs_list, market_data):
    """Weights of specs that differ in `size` (conjugate specs: also in the prior - vw / ew, VIX / EPU, mcm_scaling) for the
    same dates with ONE host pack at the largest size (`batch.pack_windows_nested`), ONE upload and ONE size sweep
    (`Batch.size_sweep`): every (window, prior) is factorised once and each size solved over its prefix of the cap-ordered
    universe.  Conjugate specs only, or Jeffreys specs only, of one (window, frequencies) family.  (date, size) pairs the pack
    cannot serve (its mask) and sizes above `_native.sweep_max_assets()` go through `_weights_for_dates` for that spec - unless
    SIZE_SWEEP_TILED is set: then, when the largest size exceeds that bound (and the sizes fit one tiled sweep), ALL sizes are
    packed once at the largest and swept with `Batch.size_sweep_tiled`.
    Returns one (weights, labels, cols, caps) per spec, each at its own size - equal to `_weights_for_dates` spec by spec
    within the solve's rounding - and remembers the conjugate ones in the cache slots `calculate_weights_for_specs` fills.
    When the pack at the largest swept size raises a ValueError - a date with fewer eligible stocks than that size, incomplete
    prices of one of its stocks - nothing is swept: every spec runs `_weights_for_dates` on its own, so the smaller sizes are
    still served and the reference's exception surfaces for the specs the reference would raise it for.
    Opt-in: nothing calls it by default."""
    specs = list(portfolio_specs_list)
    if not specs:
        return []
    conj = specs[0]["weighting_strategy"] in _CONJUGATE
    if (any((sp["weighting_strategy"] in _CONJUGATE) != conj or (not conj and sp["weighting_strategy"] != "jeffreys") for sp in specs)
            or len({_size_family(sp) for sp in specs}) != 1):
        raise ValueError("calculate_weights_for_sizes: conjugate specs, or Jeffreys specs, of equal window and frequencies expected")
    trading_dates = list(trading_dates)
    n_dates = len(trading_dates)
    members_of = _members_provider(market_data)
    N = specs[0]["rolling_window"]
    gammas = [sp["risk_aversion"] for sp in specs]
    same_gamma = all(g == gammas[0] for g in gammas)
    sizes = sorted({int(sp["size"]) for sp in specs})
    tiled = bool(SIZE_SWEEP_TILED and sizes[-1] > _native.sweep_max_assets() and len(sizes) <= _native.SWEEP_MAX_RHS
                 and sizes[-1] + len(sizes) <= _native.max_assets() + 1)
    if not tiled:
        sizes = [ks for ks in sizes if ks <= _native.sweep_max_assets()]
    swept = None
    packed = None
    if sizes:
        try:
            packed = batch.pack_windows_nested(trading_dates, specs[0], sizes, market_data, members_of=members_of)
        except ValueError as exc:                        # see the docstring: the specs decide one by one what the caller sees
            logger.warning(f"size sweep dropped ({exc}); solving the {len(specs)} specs one by one")
    if packed is not None:
        k = sizes[-1]
        kw, labels, caps, mask = packed
        n0 = w0 = None
        prior_keys = []
        if conj:
            prior_of = lambda sp: (sp["weighting_strategy"], sp["mcm_scaling"])
            prior_keys = list(dict.fromkeys(prior_of(sp) for sp in specs if sp["size"] <= k))
            n0 = np.empty((n_dates, len(prior_keys)))
            w0 = np.zeros((n_dates, len(prior_keys), len(sizes), k))
            for p, key in enumerate(prior_keys):
                sp = next(sp for sp in specs if prior_of(sp) == key)
                wanted = {int(x["size"]) for x in specs if prior_of(x) == key}
                for s, ks in enumerate(sizes):           # w0 over the prefix (ref:692-695 / 670-672); n0 does not depend on size
                    if ks in wanted:
                        w0[:, p, s, :ks], n0[:, p] = batch.prior_inputs(trading_dates, dict(sp, size=ks), market_data, caps[:, :ks])
                    else:                                # no spec asks for this pair: any finite prior does, its result is not read
                        w0[:, p, s, :ks] = 1.0 / ks
        b = _native.Batch(_native.default_device(), "conjugate" if conj else "jeffreys", k, N, kw["n_r"],
                          gammas[0] if same_gamma else 1.0, n_dates, kw.get("m") or 0)
        try:
            b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m", "w0", "n0")},
                     **(dict(w0=kw["w0"], n0=kw["n0"]) if conj else {}))
            weights, status, _ = (b.size_sweep_tiled if tiled else b.size_sweep)(sizes, n0, w0, want_aux=False)
        finally:
            b.close()
        swept = (weights, status, labels, kw["col_idx"], caps, mask, prior_keys)
    out = []
    for sp in specs:
        ks = int(sp["size"])
        if swept is None or ks not in sizes:
            res = _weights_for_dates(trading_dates, sp, market_data)
        else:
            weights, status, labels, cols, caps, mask, prior_keys = swept
            s = sizes.index(ks)
            p = prior_keys.index((sp["weighting_strategy"], sp["mcm_scaling"])) if conj else 0
            ok = mask[:, s]
            _raise_on_status(status[ok, p, s])
            w = np.ascontiguousarray(weights[:, p, s, :ks])
            if not same_gamma:
                w = 1.0 / sp["risk_aversion"] * w
            lab = [row[:ks] for row in labels]
            res = (w, lab, np.ascontiguousarray(cols[:, :ks]), np.ascontiguousarray(caps[:, :ks]))
            if not ok.all():                             # these dates' smaller universe is not the pack's prefix, or has other rows
                miss = np.flatnonzero(~ok)
                alone = _weights_for_dates([trading_dates[i] for i in miss], sp, market_data)
                for j, i in enumerate(miss):
                    res[0][i], res[1][i], res[2][i], res[3][i] = alone[0][j], alone[1][j], alone[2][j], alone[3][j]
        if conj:
            res = _fill_spec_cache([sp], trading_dates, market_data, res[0], n_dates, True, res[1], res[2], res[3])[0]
        out.append(res)
    return out


# `calculate_weights_for_windows` with a size above `_native.sweep_max_assets()`: True packs once at the longest window and
# takes one tiled window sweep (`Batch.window_sweep_tiled`) instead of one `_weights_for_dates` per spec.  Off: DESIGN.md
# section 4m holds the timings a later change decides the default from.
WINDOW_SWEEP_TILED = False


def _window_family(portfolio_spec):
    """Specs with equal (rebalancing frequency, size, window frequency) see the same universe candidates at a date;
    `rolling_window` picks a tail of the longest window's rows."""
    return tuple(portfolio_spec.get(name) for name in ("rebalancing_frequency", "size", "rolling_window_frequency"))


def calculate_weights_for_windows(trading_dates, portfolio_specs_list, market_data):
    """Weights of specs that differ in `rolling_window` (conjugate specs: also in the prior - vw / ew, VIX / EPU, mcm_scaling)
    for the same dates with ONE host pack at the longest window (`batch.pack_windows_lengths`), ONE upload and ONE window sweep
    (`Batch.window_sweep`): every daily row passes the device once, the intraday scatter is formed once per date, and each
    length is solved from a snapshot of the running Gram with its own N, n0 and risk-free offsets.  Conjugate specs only, or
    Jeffreys specs only, of one (rebalancing frequency, size, window frequency) family.  (date, length) pairs the pack cannot
    serve (its mask), a pack that raises, more than `_native.SWEEP_MAX_RHS` lengths and sizes above
    `_native.sweep_max_assets()` go through `_weights_for_dates` spec by spec, so the reference's exceptions surface where the
    reference raises them - unless WINDOW_SWEEP_TILED is set: then a size above that bound is packed the same way and swept
    with `Batch.window_sweep_tiled`.
    Returns one (weights, labels, cols, caps) per spec - equal to `_weights_for_dates` spec by spec within the solve's rounding -
    and remembers the conjugate ones in the cache slots `calculate_weights_for_specs` fills.
    Opt-in: nothing calls it by default."""
    specs = list(portfolio_specs_list)
    if not specs:
        return []
    conj = specs[0]["weighting_strategy"] in _CONJUGATE
    if (any((sp["weighting_strategy"] in _CONJUGATE) != conj or (not conj and sp["weighting_strategy"] != "jeffreys") for sp in specs)
            or len({_window_family(sp) for sp in specs}) != 1):
        raise ValueError("calculate_weights_for_windows: conjugate specs, or Jeffreys specs, of equal size and frequencies expected")
    trading_dates = list(trading_dates)
    n_dates = len(trading_dates)
    members_of = _members_provider(market_data)
    k = int(specs[0]["size"])
    gammas = [sp["risk_aversion"] for sp in specs]
    same_gamma = all(g == gammas[0] for g in gammas)
    windows = sorted({int(sp["rolling_window"]) for sp in specs})
    packed = None
    tiled = bool(WINDOW_SWEEP_TILED and k > _native.sweep_max_assets())
    if (tiled or k <= _native.sweep_max_assets()) and len(windows) <= _native.SWEEP_MAX_RHS:
        try:
            packed = batch.pack_windows_lengths(trading_dates, specs[0], windows, market_data, members_of=members_of)
        except (ValueError, AssertionError) as exc:      # the specs decide one by one what the caller sees
            logger.warning(f"window sweep dropped ({exc}); solving the {len(specs)} specs one by one")
    swept = None
    if packed is not None:
        kw, labels, caps, rows, delta, mask = packed
        n0 = w0 = None
        prior_keys = []
        if conj:
            prior_of = lambda sp: (sp["weighting_strategy"], sp["mcm_scaling"])
            prior_keys = list(dict.fromkeys(prior_of(sp) for sp in specs))
            n0 = np.empty((n_dates, len(prior_keys), len(windows)))
            w0 = np.empty((n_dates, len(prior_keys), k))
            for p, key in enumerate(prior_keys):
                sp = next(sp for sp in specs if prior_of(sp) == key)
                for l, N in enumerate(windows):          # n0 reads the length (ref:112, 265); w0 does not
                    w0[:, p], n0[:, p, l] = batch.prior_inputs(trading_dates, dict(sp, rolling_window=N), market_data, caps)
        b = _native.Batch(_native.default_device(), "conjugate" if conj else "jeffreys", k, windows[-1], kw["n_r"],
                          gammas[0] if same_gamma else 1.0, n_dates, kw.get("m") or 0)
        try:
            b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
            weights, status, _ = (b.window_sweep_tiled if tiled else b.window_sweep)(
                windows, rows, n0, w0, delta=delta if delta.any() else None, want_aux=False)
        finally:
            b.close()
        swept = (weights, status, labels, kw["col_idx"], caps, mask, prior_keys)
    out = []
    for sp in specs:
        if swept is None:
            res = _weights_for_dates(trading_dates, sp, market_data)
        else:
            weights, status, labels, cols, caps, mask, prior_keys = swept
            l = windows.index(int(sp["rolling_window"]))
            p = prior_keys.index((sp["weighting_strategy"], sp["mcm_scaling"])) if conj else 0
            ok = mask[:, l]
            _raise_on_status(status[ok, p, l])
            w = np.ascontiguousarray(weights[:, p, l])
            if not same_gamma:
                w = 1.0 / sp["risk_aversion"] * w
            res = (w, [list(row) for row in labels], cols.copy(), caps.copy())
            if not ok.all():                             # these dates' shorter window has another universe, or trips a check
                miss = np.flatnonzero(~ok)
                alone = _weights_for_dates([trading_dates[i] for i in miss], sp, market_data)
                for j, i in enumerate(miss):
                    res[0][i], res[1][i], res[2][i], res[3][i] = alone[0][j], alone[1][j], alone[2][j], alone[3][j]
        if conj:
            res = _fill_spec_cache([sp], trading_dates, market_data, res[0], n_dates, True, res[1], res[2], res[3])[0]
        out.append(res)
    return out


# `calculate_weights_for_grid` with a largest size above `_native.sweep_max_assets()`: True packs every requested size once at
# the largest (and the longest window) and takes one tiled grid sweep (`Batch.grid_sweep_tiled`) - the sizes below that bound
# are then prefixes of the same sweep - instead of one `_weights_for_dates` per spec above it.  Off: DESIGN.md section 4o holds
# the timings a later change decides the default from.
GRID_SWEEP_TILED = False


def _grid_family(portfolio_spec):
    """Specs with equal (rebalancing frequency, window frequency): `size` picks a prefix of the cap-ordered universe and
    `rolling_window` a tail of the longest window's rows."""
    return tuple(portfolio_spec.get(name) for name in ("rebalancing_frequency", "rolling_window_frequency"))


def _grid_sweep_stage(trading_dates, specs, market_data, want_weights=True, keep_open=False):
    """The pack-and-sweep stage of `calculate_weights_for_grid` (and of `backtest_portfolios_grid`): the family check, ONE host
    pack at (largest size, longest window), ONE upload and ONE grid sweep.  Returns (sizes, windows, conj, same_gamma, swept, b):
    `swept` = (weights, status, labels, cols, caps, mask, prior_keys), or None when no sweep serves the specs (the caller then
    solves them one by one); `want_weights=False` leaves the weights on the device (None in their place).  `keep_open`: `b` is
    the batch, still open - its results are on the device and the caller closes it - otherwise None."""
    conj = specs[0]["weighting_strategy"] in _CONJUGATE
    if (any((sp["weighting_strategy"] in _CONJUGATE) != conj or (not conj and sp["weighting_strategy"] != "jeffreys") for sp in specs)
            or len({_grid_family(sp) for sp in specs}) != 1):
        raise ValueError("calculate_weights_for_grid: conjugate specs, or Jeffreys specs, of equal frequencies expected")
    n_dates = len(trading_dates)
    members_of = _members_provider(market_data)
    gammas = [sp["risk_aversion"] for sp in specs]
    same_gamma = all(g == gammas[0] for g in gammas)
    windows = sorted({int(sp["rolling_window"]) for sp in specs})
    sizes = sorted({int(sp["size"]) for sp in specs})
    tiled = bool(GRID_SWEEP_TILED and sizes[-1] > _native.sweep_max_assets() and len(sizes) <= _native.SWEEP_MAX_RHS
                 and len(windows) <= _native.SWEEP_MAX_RHS and sizes[-1] + len(sizes) <= _native.max_assets() + 1)
    if not tiled:
        sizes = [ks for ks in sizes if ks <= _native.sweep_max_assets()]
    packed = None
    if sizes and len(sizes) <= _native.SWEEP_MAX_RHS and len(windows) <= _native.SWEEP_MAX_RHS:
        try:
            packed = batch.pack_windows_grid(trading_dates, specs[0], sizes, windows, market_data, members_of=members_of)
        except (ValueError, AssertionError) as exc:      # the specs decide one by one what the caller sees
            logger.warning(f"grid sweep dropped ({exc}); solving the {len(specs)} specs one by one")
    if packed is None:
        return sizes, windows, conj, same_gamma, None, None
    k = sizes[-1]
    kw, labels, caps, rows, delta, mask = packed
    n0 = w0 = None
    prior_keys = []
    if conj:
        prior_of = lambda sp: (sp["weighting_strategy"], sp["mcm_scaling"])
        prior_keys = list(dict.fromkeys(prior_of(sp) for sp in specs if sp["size"] <= k))
        n0 = np.empty((n_dates, len(prior_keys), len(windows)))
        w0 = np.zeros((n_dates, len(prior_keys), len(sizes), k))
        for p, key in enumerate(prior_keys):
            sp = next(sp for sp in specs if prior_of(sp) == key)
            wanted = {int(x["size"]) for x in specs if prior_of(x) == key}
            for l, N in enumerate(windows):          # n0 reads the length (ref:112, 265), not the size
                n0[:, p, l] = batch.prior_inputs(trading_dates, dict(sp, size=k, rolling_window=N), market_data, caps)[1]
            # w0 over the prefix (ref:692-695 / 670-672) reads the caps alone - neither the length nor the dates: one date is
            # passed so that the n0 it returns next to it is not computed W times per size
            for s, ks in enumerate(sizes):
                if ks in wanted:
                    w0[:, p, s, :ks] = batch.prior_inputs(trading_dates[:1], dict(sp, size=ks), market_data, caps[:, :ks])[0]
                else:                                # no spec asks for this pair: any finite prior does, its result is not read
                    w0[:, p, s, :ks] = 1.0 / ks
    b = _native.Batch(_native.default_device(), "conjugate" if conj else "jeffreys", k, windows[-1], kw["n_r"],
                      gammas[0] if same_gamma else 1.0, n_dates, kw.get("m") or 0)
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        weights, status, _ = (b.grid_sweep_tiled if tiled else b.grid_sweep)(
            sizes, windows, rows, n0, w0, delta=delta if delta.any() else None, want_aux=False, want_weights=want_weights)
    except BaseException:
        b.close()
        raise
    if not keep_open:
        b.close()
        b = None
    return sizes, windows, conj, same_gamma, (weights, status, labels, kw["col_idx"], caps, mask, prior_keys), b


def calculate_weights_for_grid(trading_dates, portfolio_specs_list, market_data):
    """Weights of specs that differ in `size` AND in `rolling_window` (conjugate specs: also in the prior - vw / ew, VIX / EPU,
    mcm_scaling) for the same dates with ONE host pack at (largest size, longest window) (`batch.pack_windows_grid`), ONE upload
    and ONE grid sweep (`Batch.grid_sweep`): every daily row passes the device once, every (date, prior, length) is factorised
    once at the largest size and each size solved over its prefix.  Conjugate specs only, or Jeffreys specs only, of one
    (rebalancing frequency, window frequency) family.  (date, size, length) triples the pack cannot serve (its mask), sizes
    above `_native.sweep_max_assets()`, more than `_native.SWEEP_MAX_RHS` sizes or lengths and a pack that raises go through
    `_weights_for_dates` spec by spec, so the reference's exceptions surface where the reference raises them - unless
    GRID_SWEEP_TILED is set: then, when the largest size exceeds that bound (and the sizes and lengths fit one tiled sweep), ALL
    sizes are packed once at the largest and swept with `Batch.grid_sweep_tiled`.
    Returns one (weights, labels, cols, caps) per spec, each at its own size - equal to `_weights_for_dates` spec by spec
    within the solve's rounding - and remembers the conjugate ones in the cache slots `calculate_weights_for_specs` fills.
    Opt-in: nothing calls it by default."""
    specs = list(portfolio_specs_list)
    if not specs:
        return []
    trading_dates = list(trading_dates)
    n_dates = len(trading_dates)
    sizes, windows, conj, same_gamma, swept, _ = _grid_sweep_stage(trading_dates, specs, market_data)
    out = []
    for sp in specs:
        ks = int(sp["size"])
        if swept is None or ks not in sizes:
            res = _weights_for_dates(trading_dates, sp, market_data)
        else:
            weights, status, labels, cols, caps, mask, prior_keys = swept
            s, l = sizes.index(ks), windows.index(int(sp["rolling_window"]))
            p = prior_keys.index((sp["weighting_strategy"], sp["mcm_scaling"])) if conj else 0
            ok = mask[:, s, l]
            _raise_on_status(status[ok, p, l, s])
            w = np.ascontiguousarray(weights[:, p, l, s, :ks])
            if not same_gamma:
                w = 1.0 / sp["risk_aversion"] * w
            lab = [row[:ks] for row in labels]
            res = (w, lab, cols[:, :ks].copy(), caps[:, :ks].copy())      # (copies: several specs share a size, a fallback writes)
            if not ok.all():                             # these dates' spec is not the pack's prefix and suffix, or trips a check
                miss = np.flatnonzero(~ok)
                alone = _weights_for_dates([trading_dates[i] for i in miss], sp, market_data)
                for j, i in enumerate(miss):
                    res[0][i], res[1][i], res[2][i], res[3][i] = alone[0][j], alone[1][j], alone[2][j], alone[3][j]
        if conj:
            res = _fill_spec_cache([sp], trading_dates, market_data, res[0], n_dates, True, res[1], res[2], res[3])[0]
        out.append(res)
    return out


def _replicated_weights(kw, priors, n_specs, k, N, gamma):
    """Every window once per spec in ONE device batch of n_specs x n_dates windows."""
    per_window = ("row_idx", "n_rows", "col_idx", "rf_adj", "hf_row_idx", "hf_count")
    big = {key: (np.concatenate([val] * n_specs, axis=0) if key in per_window and val is not None else val)
           for key, val in kw.items()}
    big["w0"] = np.concatenate([p[0] for p in priors], axis=0)
    big["n0"] = np.concatenate([p[1] for p in priors], axis=0)
    # 1/gamma is the last factor of ref:836: with different risk aversions in one batch the device runs with
    # gamma = 1 and the same multiplication happens here (same rounding: (1/gamma) * x in both places)
    weights, status, _ = _device_posterior_batch("conjugate", k, N, gamma, big)
    _raise_on_status(status)
    return weights


def _fill_spec_cache(specs, trading_dates, market_data, weights, n_dates, same_gamma, labels, cols, caps):
    """Cut the [n_specs * n_dates x k] weights into one result per spec and remember each in its cache slot."""
    out = []
    for i, sp in enumerate(specs):
        w = weights[i * n_dates:(i + 1) * n_dates]
        if not same_gamma:
            w = 1.0 / sp["risk_aversion"] * w
        res = (w, labels, cols, caps)
        cache, key, owners = _cache_slot(sp, trading_dates, market_data)
        if len(cache) > 64:
            cache.clear()
        cache[key] = (res, owners)
        out.append(res)
    return out


# Cross-spec prefetch of `backtest_portfolio` (off with TP_PREFETCH_SIBLINGS=0): at most this many windows per batch,
# siblings beyond it wait for their own call
PREFETCH_SIBLINGS = os.environ.get("TP_PREFETCH_SIBLINGS", "1") not in ("0", "")
PREFETCH_MAX_WINDOWS = int(os.environ.get("TP_PREFETCH_MAX_WINDOWS", "65536"))


def _prefetch_siblings(portfolio_spec, rebalance_dates, market_data):
    """`backtest_portfolio` is called once per spec (src/main.py:48): when the spec is a conjugate spec of the grid
    `portfolio_specs.create_portfolio_specs()` returned last, solve its conjugate siblings with the same windows in
    the same device batch, so that their own `backtest_portfolio` calls find the weights ready.

    Only an optimisation, so it never changes what the call itself does: the batch is capped
    (`PREFETCH_MAX_WINDOWS` windows: the index arrays are replicated per spec), and ANY failure of the joint batch - a
    sibling whose market data is missing or whose prior strength raises - is logged and dropped: the spec then runs on
    its own, and the sibling's problem surfaces in the sibling's own `backtest_portfolio`, where the reference's loop
    would raise it."""
    if not PREFETCH_SIBLINGS or portfolio_spec["weighting_strategy"] not in _CONJUGATE:
        return
    cache, key, owners = _cache_slot(portfolio_spec, rebalance_dates, market_data)
    if key in cache and cache[key][1][0] is owners[0] and cache[key][1][1] is owners[1]:
        return
    family = _batch_family(portfolio_spec)
    siblings = [sp for sp in portfolio_specs.last_grid().values()
                if sp["weighting_strategy"] in _CONJUGATE and _batch_family(sp) == family
                and _spec_cache_key(sp) != _spec_cache_key(portfolio_spec) and sp.get("risk_aversion")]
    room = PREFETCH_MAX_WINDOWS // max(len(rebalance_dates), 1) - 1
    siblings = siblings[:max(room, 0)]
    if not siblings:
        return
    try:
        calculate_weights_for_specs(rebalance_dates, [portfolio_spec] + siblings, market_data)
    except Exception as exc:      # noqa: BLE001 - see the docstring: the single-spec path decides what the caller sees
        logger.warning(f"cross-spec prefetch dropped ({type(exc).__name__}: {exc}); solving {portfolio_spec.get('display_name')} alone")


def calculate_portfolio_weights_batch(trading_dates, portfolio_spec, market_data):
    """Weights for MANY rebalancing dates with one device call (the batch-native form of ref:941).

    Host side: `batch.pack_windows` turns the dates into panel + row/column-index arrays without
    per-date pandas work; device side: one `posterior_batch` launch."""
    strategy = portfolio_spec["weighting_strategy"]
    if strategy in ("vw", "ew"):
        return [calculate_portfolio_weights(d, portfolio_spec, market_data) for d in trading_dates]
    if not trading_dates:
        if strategy in _OUT_OF_SCOPE:
            _not_in_scope(f"calculate_{strategy}_portfolio")()
        return []
    weights, labels, _, _ = _weights_for_dates(trading_dates, portfolio_spec, market_data)
    return [pd.DataFrame({"Weight": weights[i]}, index=pd.Index(labels[i], name="Stock")) for i in range(len(labels))]


def calculate_posterior_scale_matrices_batch(trading_dates, portfolio_spec, market_data):
    """The posterior scale matrix of MANY rebalancing dates with one device batch: S1 = S0 + T (ref:358) for the conjugate
    specs, J = T - t t'/N (ref:600-601) for `jeffreys` - the matrices the weights of `calculate_portfolio_weights_batch`
    factorise, stored by the same kernels (`Batch.keep_posterior`).  One k x k DataFrame per date; index and columns are
    that date's tickers in the order of its weights.  Replaces a per-date loop of `calculate_conjugate_posterior_S`.
    One device even with sharding opted in."""
    strategy = portfolio_spec["weighting_strategy"]
    if strategy not in _CONJUGATE and strategy != "jeffreys":
        raise ValueError(f"calculate_posterior_scale_matrices_batch: no posterior scale matrix for strategy {strategy!r} "
                         "(conjugate strategies and 'jeffreys' have one)")
    trading_dates = list(trading_dates)
    if not trading_dates:
        return []
    k, N = portfolio_spec["size"], portfolio_spec["rolling_window"]
    gamma = portfolio_spec.get("risk_aversion") or 1.0           # the matrices do not depend on it
    kw, labels = batch.pack_windows(trading_dates, portfolio_spec, market_data, members_of=_members_provider(market_data))
    _, _, _, M = _native.posterior_batch("conjugate" if strategy in _CONJUGATE else "jeffreys", k, N, gamma, **kw,
                                         want_aux=False, want_posterior=True)
    return [pd.DataFrame(M[i], index=pd.Index(labels[i]), columns=pd.Index(labels[i])) for i in range(len(labels))]


def _members_provider(market_data):
    """Index membership per date for the batch packer: None = every column (synthetic panels)."""
    provider = market_data.get("index_constituents") if isinstance(market_data, dict) else None
    if callable(provider):
        return provider
    try:
        import data_handling  # the reference's data layer, if the caller has it on sys.path
        return lambda ts: data_handling.extract_unique_tickers(ts, ts)
    except Exception:
        return None


def calculate_portfolio_weights(trading_date_ts, portfolio_spec, market_data):
    """Strategy dispatch for one date (ref:941-1052); rows ordered by market cap, index 'Stock'."""
    strategy = portfolio_spec["weighting_strategy"]
    if strategy == "vw":
        uni = _Universe(trading_date_ts, portfolio_spec, market_data)
        return calculate_value_weighted_portfolio(portfolio_spec, trading_date_ts, uni.caps)
    if strategy == "ew":
        uni = _Universe(trading_date_ts, portfolio_spec, market_data)
        return calculate_equally_weighted_portfolio(portfolio_spec, uni.prices)
    return calculate_portfolio_weights_batch([trading_date_ts], portfolio_spec, market_data)[0]


# ======================================================================================================
# backtest engine (ref:1054-1238)
def compute_portfolio_turnover(portfolio_weights_before_df, portfolio_weights_after_df):
    """Half the L1 change of the weights, the risk-free position included (ref:1054-1075)."""
    both = portfolio_weights_before_df.merge(portfolio_weights_after_df, how="outer", left_index=True,
                                             right_index=True, suffixes=("_before", "_after")).fillna(0)
    traded = (both["Weight_before"] - both["Weight_after"]).abs().sum()
    cash = abs(portfolio_weights_before_df["Weight"].sum() - portfolio_weights_after_df["Weight"].sum())
    return (traded + cash) / 2


def calculate_average_distance_to_comparison_portfolio(portfolio_weights_df, portfolio_spec, trading_date_ts,
                                                       market_data, comparison_portfolio_weighting_strategy):
    """Mean absolute distance to the value-weighted portfolio of the same universe (ref:1077-1104)."""
    if comparison_portfolio_weighting_strategy != "vw":
        raise ValueError("Unknown comparison portfolio.")
    comparison_spec = {"size": portfolio_spec["size"], "rebalancing_frequency": portfolio_spec["rebalancing_frequency"],
                       "rolling_window": portfolio_spec["rolling_window"],
                       "rolling_window_frequency": portfolio_spec["rolling_window_frequency"],
                       "weighting_strategy": "vw"}
    comparison = calculate_portfolio_weights(trading_date_ts, comparison_spec, market_data)
    if not portfolio_weights_df.index.equals(comparison.index):
        raise ValueError("The portfolios do not match exactly in terms of stocks.")
    scaling = portfolio_spec["risk_aversion"] if portfolio_spec.get("risk_aversion") is not None else 1
    return np.abs(portfolio_weights_df * scaling - comparison).mean().item()


def rebalancing_schedule(trading_dates, rebalancing_frequency):
    """Rebalancing dates of a backtest (ref:1166-1176): they depend on the date list only, which is
    what lets `backtest_portfolio` solve all windows in one batch before replaying the P&L."""
    out, last = [], None
    for ts in trading_dates:
        if last is None or rebalancing_frequency == "daily":
            hit = True
        elif rebalancing_frequency == "weekly":
            hit = ts.weekday() == 2 or (ts - last).days > 7
        elif rebalancing_frequency == "monthly":
            hit = ts.month != last.month
        else:
            logger.error("Unknown rebalancing frequency.")
            raise ValueError("Unknown rebalancing frequency.")
        if hit:
            out.append(ts)
            last = ts
    return out


class Portfolio:
    """Daily P&L, weight drift, rebalancing, turnover and weight metrics (ref:1106-1219)."""

    def __init__(self, ts_start_date, portfolio_spec, precomputed_weights=None):
        self.ts_start_date = ts_start_date
        self.portfolio_spec = portfolio_spec
        self.portfolio_simple_returns_series = pd.Series(dtype="float64", name=portfolio_spec["display_name"])
        self.portfolio_turnover_series = pd.Series(dtype="float64", name=portfolio_spec["display_name"])
        self.portfolio_weights_metrics_df = pd.DataFrame(dtype="float64")
        self.last_rebalance_date_ts = None
        self._precomputed = precomputed_weights or {}

    def get_portfolio_simple_returns(self):
        return self.portfolio_simple_returns_series

    def get_portfolio_turnover(self):
        return self.portfolio_turnover_series

    def get_portfolio_weights_metrics(self):
        return self.portfolio_weights_metrics_df

    def _mark_to_market(self, trading_date_ts, market_data):
        w = self.portfolio_weights_df["Weight"]
        returns = market_data["stock_simple_returns_df"].loc[trading_date_ts].reindex(self.portfolio_weights_df.index)
        rf_annual = market_data["risk_free_rate_df"].asof(trading_date_ts).iloc[0]
        rf_daily = (rf_annual + 1) ** (1 / 252) - 1
        cash = 1 - w.sum()
        self.portfolio_simple_returns_series[trading_date_ts] = (returns * w).sum() + cash * rf_daily   # ref:1137-1145
        cash_after = cash * (1 + rf_daily)
        drifted = w * (1 + returns)
        total = drifted.sum() + cash_after
        self.portfolio_weights_df["Weight"] = drifted / total                                          # ref:1152-1159
        if abs((self.portfolio_weights_df["Weight"].values.sum() + cash_after / total) - 1) > 1e-5:
            logger.error("Weights do not sum to 1.")
            raise ValueError("Weights do not sum to 1.")

    def _is_rebalance_day(self, trading_date_ts):
        freq = self.portfolio_spec["rebalancing_frequency"]
        if self.last_rebalance_date_ts is None or freq == "daily":
            return True
        if freq == "weekly":
            return trading_date_ts.weekday() == 2 or (trading_date_ts - self.last_rebalance_date_ts).days > 7
        if freq == "monthly":
            return trading_date_ts.month != self.last_rebalance_date_ts.month
        logger.error("Unknown rebalancing frequency.")
        raise ValueError("Unknown rebalancing frequency.")

    def update_portfolio(self, trading_date_ts, market_data):
        if self.ts_start_date != trading_date_ts:
            self._mark_to_market(trading_date_ts, market_data)
        if not self._is_rebalance_day(trading_date_ts):
            return
        first = self.last_rebalance_date_ts is None
        before = None if first else self.portfolio_weights_df.copy()
        if trading_date_ts in self._precomputed:
            self.portfolio_weights_df = self._precomputed[trading_date_ts].copy()
        else:
            self.portfolio_weights_df = calculate_portfolio_weights(trading_date_ts, self.portfolio_spec, market_data)
        distance = calculate_average_distance_to_comparison_portfolio(self.portfolio_weights_df, self.portfolio_spec,
                                                                      trading_date_ts, market_data, "vw")
        w = self.portfolio_weights_df["Weight"]
        row = pd.DataFrame({"max_long": [w[w > 0].max()], "max_short": [w[w < 0].min()],
                            "avg_long": [w[w > 0].mean()], "avg_short": [w[w < 0].mean()],
                            "average_distance_to_comparison_portfolio": [distance]}, index=[trading_date_ts])
        self.portfolio_weights_metrics_df = pd.concat([self.portfolio_weights_metrics_df, row])
        if not first:
            turnover = compute_portfolio_turnover(before, self.portfolio_weights_df)
            self.portfolio_turnover_series[trading_date_ts] = turnover
            self.portfolio_simple_returns_series[trading_date_ts] -= self.portfolio_spec["turnover_cost"] / 10000 * turnover
        logger.info(f"Portfolio size {trading_date_ts}: {len(self.portfolio_weights_df.index)}")
        self.last_rebalance_date_ts = trading_date_ts


def _rf_asof(risk_free_rate_df, trading_dates):
    """`risk_free_rate_df.asof(ts).iloc[0]` for every date (ref:1139): the last row at or before ts that has no
    NaN (DataFrame.asof skips NaN rows)."""
    rf = risk_free_rate_df.sort_index()
    vals = rf.to_numpy(dtype=np.float64).reshape(len(rf), -1)
    ok = ~np.isnan(vals).any(axis=1)
    idx_ns = rf.index.values.astype("datetime64[ns]").astype(np.int64)[ok]
    first = vals[ok][:, 0]
    d = np.array([pd.Timestamp(ts).value for ts in trading_dates], dtype=np.int64)
    pos = np.searchsorted(idx_ns, d, side="right") - 1
    return np.where(pos >= 0, first[np.maximum(pos, 0)], np.nan)


def _replay_backtest(trading_dates, rebalance_dates, weights, cols, caps, tickers, portfolio_spec, market_data):
    """The daily loop of ref:1127-1219 (mark to market, drift, rebalance, turnover ref:1054-1075, weight metrics,
    distance to the value-weighted portfolio ref:1077-1104) over plain arrays: the weights of every rebalancing
    date are already in hand, so a day costs a few k-vector operations instead of a dozen DataFrame slices.
    Same operations in the same order as `Portfolio.update_portfolio`, NaN-skipping sums where pandas skips."""
    name = portfolio_spec["display_name"]
    K = len(tickers)
    sr = market_data["stock_simple_returns_df"]
    missing = [ts for ts in trading_dates[1:] if ts not in sr.index]
    if missing:
        raise KeyError(missing[0])                                        # ref:1134 `.loc[trading_date_ts]`
    S = sr.reindex(index=pd.DatetimeIndex(trading_dates), columns=tickers).to_numpy(dtype=np.float64)
    rf_daily_all = (_rf_asof(market_data["risk_free_rate_df"], trading_dates) + 1) ** (1 / 252) - 1     # ref:1140
    scaling = portfolio_spec["risk_aversion"] if portfolio_spec.get("risk_aversion") is not None else 1
    cost = portfolio_spec["turnover_cost"]
    reb_index = {ts: j for j, ts in enumerate(rebalance_dates)}
    n_days = len(trading_dates)
    returns = np.full(n_days, np.nan)
    turnover = np.full(len(rebalance_dates), np.nan)
    metrics = np.full((len(rebalance_dates), 5), np.nan)
    w = held = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for di, ts in enumerate(trading_dates):
            if di > 0:
                r, rf_daily = S[di, held], rf_daily_all[di]
                cash = 1 - np.nansum(w)
                returns[di] = np.nansum(r * w) + cash * rf_daily                    # ref:1137-1145
                cash_after = cash * (1 + rf_daily)
                drifted = w * (1 + r)
                total = np.nansum(drifted) + cash_after
                w = drifted / total                                                 # ref:1152-1159
                if abs((w.sum() + cash_after / total) - 1) > 1e-5:
                    logger.error("Weights do not sum to 1.")
                    raise ValueError("Weights do not sum to 1.")
            j = reb_index.get(ts)
            if j is None:
                continue
            before_w, before_held = w, held
            w, held = weights[j].astype(np.float64, copy=True), cols[j]
            vw = caps[j] / np.nansum(caps[j])                                       # ref:692-695
            pos_w, neg_w = w[w > 0], w[w < 0]
            metrics[j] = (pos_w.max() if pos_w.size else np.nan, neg_w.min() if neg_w.size else np.nan,
                          pos_w.mean() if pos_w.size else np.nan, neg_w.mean() if neg_w.size else np.nan,
                          np.nanmean(np.abs(w * scaling - vw)))                      # ref:1100-1104
            if before_w is not None:
                dense_b, dense_a = np.zeros(K), np.zeros(K)                         # outer merge + fillna(0), ref:1062-1066
                dense_b[before_held] = np.nan_to_num(before_w, nan=0.0)
                dense_a[held] = np.nan_to_num(w, nan=0.0)
                union = np.union1d(before_held, held)
                traded = np.abs(dense_b[union] - dense_a[union]).sum()
                turnover[j] = (traded + abs(np.nansum(before_w) - np.nansum(w))) / 2    # ref:1068-1075
                returns[di] -= cost / 10000 * turnover[j]                           # ref:1212
    days = pd.DatetimeIndex(trading_dates)
    reb = pd.DatetimeIndex(rebalance_dates)
    return {"portfolio_simple_returns_series": pd.Series(returns[1:], index=days[1:], name=name, dtype="float64"),
            "portfolio_turnover_series": pd.Series(turnover[1:], index=reb[1:], name=name, dtype="float64"),
            "portfolio_weights_metrics_df": pd.DataFrame(
                metrics, index=reb, dtype="float64",
                columns=["max_long", "max_short", "avg_long", "avg_short", "average_distance_to_comparison_portfolio"])}


# `backtest_portfolios` replays its specs on the device (`replay_backtests_device`: one call per group of specs with the same
# rebalancing frequency and ticker list) instead of one host loop per spec.  Opt-in: the host replay is the default and the
# yardstick; the two agree to the rounding of their summation orders.
DEVICE_REPLAY = False


def replay_backtests_device(trading_dates, rebalance_dates, items, market_data, tickers=None, device=None):
    """`_replay_backtest` for MANY specs in ONE device call (`_native.Device.replay`): `items` is a list of
    (weights [R x k], cols [R x k], caps [R x k], portfolio_spec) over the same trading dates, rebalancing dates and ticker
    list (`tickers`; default: the panels' of the first spec's window frequency).  Returns, per item, the dict
    `_replay_backtest` returns - same indices, names, dtypes and columns.  Arrays that are the same object (the universe and
    caps of one spec family, the passive weights) are packed and uploaded once."""
    items = list(items)
    if not items:
        return []
    _dev, (returns, turnover, metrics, status, _bad_day) = _replay_items(trading_dates, rebalance_dates, items, market_data,
                                                                         tickers, device)
    if np.any(np.asarray(status) != 0):
        logger.error("Weights do not sum to 1.")
        raise ValueError("Weights do not sum to 1.")
    return _device_replay_results(trading_dates, rebalance_dates, [item[3] for item in items], returns, turnover, metrics)


def summarise_backtests_device(trading_dates, rebalance_dates, items, market_data, turnover_costs, tickers=None, device=None):
    """The metrics table of ref:464-701 for the `items` of `replay_backtests_device` at every trading cost of `turnover_costs`
    (basis points), without the P&L ever leaving the device: ONE replay at cost 0 (a cost never touches the holdings, ref:1212;
    the specs' own `turnover_cost` is not read), its results kept on the device (`download=False`), then
    `Device.replay_summary` over the costs; 256 bytes per (spec, cost) come down.  Returns the frame of
    `portfolio_evaluation.performance_table`, indexed by (display_name, cost); Prob. Sharpe against the 'S&P 500' column of
    market_data["sp500_simple_returns_df"] when the market data has one (ref:555), NaN otherwise.  "Weights do not sum to 1."
    raises the reference's ValueError."""
    items = list(items)
    if not items:
        return portfolio_evaluation.performance_table(np.zeros((0, len(turnover_costs), _native.SUMMARY_STATS)),
                                                      np.zeros((0, len(turnover_costs)), dtype=np.int32), trading_dates, [],
                                                      turnover_costs)
    dev, _none = _replay_items(trading_dates, rebalance_dates, items, market_data, tickers, device, cost_all=0.0, download=False)
    table = _summary_table(dev, trading_dates, [item[3] for item in items], market_data, turnover_costs)
    if table is None:
        logger.error("Weights do not sum to 1.")
        raise ValueError("Weights do not sum to 1.")
    return table


def _summary_table(dev, trading_dates, specs, market_data, turnover_costs):
    """`Device.replay_summary` of the replay just queued on `dev` and the frame of `performance_table` for `specs`; None when
    the replay set a status (the caller raises what that status means)."""
    rates = market_data["risk_free_rate_df"]
    if "DTB3" not in rates:                                   # (`_rf_asof` reads the first column, whatever its name)
        rates = rates.rename(columns={rates.columns[0]: "DTB3"})
    rf_excess = portfolio_evaluation.rf_excess_for(trading_dates, rates)
    stats, status = dev.replay_summary(turnover_costs, rf_excess)
    if np.any(status == _native.SUMMARY_NO_REPLAY):
        return None
    benchmark = None
    sp500 = market_data.get("sp500_simple_returns_df")
    if sp500 is not None:
        series = sp500.iloc[:, 0].reindex(pd.DatetimeIndex(trading_dates)[1:])
        benchmark = (series.to_numpy(dtype=np.float64) - rf_excess[1:])
    return portfolio_evaluation.performance_table(stats, status, trading_dates, [sp["display_name"] for sp in specs],
                                                  turnover_costs, benchmark_excess=benchmark)


def _replay_items(trading_dates, rebalance_dates, items, market_data, tickers, device, cost_all=None, download=True):
    """Packs `items` and replays them in one `Device.replay`: (device, what the replay returned).  `cost_all`: one trading cost
    for every item instead of its spec's."""
    if tickers is None:
        tickers = batch.panels_for(market_data, items[0][3]["rolling_window_frequency"]).tickers
    S, rf_daily, reb_day = _device_replay_inputs(trading_dates, rebalance_dates, market_data, tickers)
    R = len(rebalance_dates)
    w_parts, c_parts, p_parts, w_at, u_at = [], [], [], {}, {}
    w_len = u_len = 0
    ks, scaling, cost, w_off, u_off = [], [], [], [], []
    for weights, cols, caps, spec in items:
        k = int(np.shape(cols)[1])
        if np.shape(weights) != (R, k) or np.shape(cols) != (R, k) or np.shape(caps) != (R, k):
            raise ValueError(f"{spec['display_name']}: weights, cols and caps of shape ({R}, k) expected, got "
                             f"{np.shape(weights)}, {np.shape(cols)}, {np.shape(caps)}")
        if id(weights) not in w_at:
            w_at[id(weights)] = w_len
            w_parts.append(np.ascontiguousarray(weights, dtype=np.float64).reshape(-1))
            w_len += R * k
        if (id(cols), id(caps)) not in u_at:
            u_at[(id(cols), id(caps))] = u_len
            c_parts.append(np.ascontiguousarray(cols, dtype=np.int32).reshape(-1))
            p_parts.append(np.ascontiguousarray(caps, dtype=np.float64).reshape(-1))
            u_len += R * k
        ks.append(k)
        scaling.append(spec["risk_aversion"] if spec.get("risk_aversion") is not None else 1)
        cost.append(spec["turnover_cost"] if cost_all is None else cost_all)
        w_off.append(w_at[id(weights)])
        u_off.append(u_at[(id(cols), id(caps))])
    ks = np.array(ks, dtype=np.int32)
    stride = ks.astype(np.int64)
    dev = device if device is not None else _native.default_device()
    keep = {} if download else {"download": False}            # (the downloading call is the one `device` objects always took)
    return dev, dev.replay(
        S, rf_daily, reb_day, len(tickers), ks, np.array(scaling, dtype=np.float64), np.array(cost, dtype=np.float64),
        np.array(w_off, dtype=np.int64), stride, np.array(u_off, dtype=np.int64), stride,
        np.concatenate(w_parts), np.concatenate(c_parts), np.concatenate(p_parts), **keep)


def _device_replay_inputs(trading_dates, rebalance_dates, market_data, tickers):
    """(S [D x K] simple returns over `tickers`, rf_daily [D], reb_day [R]) as the device replays read them."""
    sr = market_data["stock_simple_returns_df"]
    missing = [ts for ts in trading_dates[1:] if ts not in sr.index]
    if missing:
        raise KeyError(missing[0])                                        # ref:1134 `.loc[trading_date_ts]`
    S = sr.reindex(index=pd.DatetimeIndex(trading_dates), columns=tickers).to_numpy(dtype=np.float64)
    rf_daily = (_rf_asof(market_data["risk_free_rate_df"], trading_dates) + 1) ** (1 / 252) - 1         # ref:1140
    day_of = {ts: d for d, ts in enumerate(trading_dates)}
    reb_day = np.array([day_of[ts] for ts in rebalance_dates], dtype=np.int32)
    return S, rf_daily, reb_day


def _device_replay_results(trading_dates, rebalance_dates, specs, returns, turnover, metrics):
    """The dicts of `_replay_backtest`, one per spec, from a device replay's arrays."""
    days = pd.DatetimeIndex(trading_dates)
    reb = pd.DatetimeIndex(rebalance_dates)
    out = []
    for p, spec in enumerate(specs):
        name = spec["display_name"]
        out.append({"portfolio_simple_returns_series": pd.Series(returns[p, 1:], index=days[1:], name=name, dtype="float64"),
                    "portfolio_turnover_series": pd.Series(turnover[p, 1:], index=reb[1:], name=name, dtype="float64"),
                    "portfolio_weights_metrics_df": pd.DataFrame(
                        metrics[p], index=reb, dtype="float64",
                        columns=["max_long", "max_short", "avg_long", "avg_short", "average_distance_to_comparison_portfolio"])})
    return out


def _grid_replay_plan(specs, sizes, windows, prior_keys, mask, k):
    """Where every spec of a grid family reads its weights in a grid sweep's results on the device - weights [W x P x L x S x k],
    status [W x P x L x S], P = len(prior_keys) (Jeffreys: no keys, P = 1) - and which (spec, date) pairs the sweep does not
    serve.  A pure function (no device, no market data).  Spec i with size sizes[s], window windows[l] and prior p reads, at
    date j, the row at w_off[i] + j * w_stride[i] = ((j P + p) L + l) S + s) k and the status at s_off[i] + j * s_stride[i];
    `w_scale[i]` is 1.0 when the risk aversions agree and 1.0 / risk_aversion otherwise (the sweep then ran with gamma = 1).
    The dates `mask[:, s, l]` does not serve, and every date of a spec whose size is outside `sizes`, become patches: their
    offsets are 0 with stride 0 for such a spec.  Returns a dict of arrays: w_off, w_stride, s_off, s_stride (int64 [n]),
    w_scale (float64 [n]), swept (bool [n]: the spec's size is in the sweep) and patch_port (int64), patch_date (int32), sorted
    by (spec, date)."""
    specs = list(specs)
    mask = np.asarray(mask, dtype=bool)
    W = mask.shape[0]
    P, L, S = max(len(prior_keys), 1), len(windows), len(sizes)
    gammas = [sp["risk_aversion"] for sp in specs]
    same_gamma = all(g == gammas[0] for g in gammas)
    n = len(specs)
    plan = {"w_off": np.zeros(n, dtype=np.int64), "w_stride": np.zeros(n, dtype=np.int64),
            "s_off": np.zeros(n, dtype=np.int64), "s_stride": np.zeros(n, dtype=np.int64),
            "w_scale": np.ones(n, dtype=np.float64), "swept": np.zeros(n, dtype=bool)}
    patch_port, patch_date = [], []
    for i, sp in enumerate(specs):
        ks = int(sp["size"])
        if not same_gamma:
            plan["w_scale"][i] = 1.0 / sp["risk_aversion"]
        if ks not in sizes:
            missed = range(W)
        else:
            s, l = sizes.index(ks), windows.index(int(sp["rolling_window"]))
            p = prior_keys.index((sp["weighting_strategy"], sp["mcm_scaling"])) if prior_keys else 0
            entry = (p * L + l) * S + s
            plan["swept"][i] = True
            plan["s_off"][i], plan["s_stride"][i] = entry, P * L * S
            plan["w_off"][i], plan["w_stride"][i] = entry * k, P * L * S * k
            missed = np.flatnonzero(~mask[:, s, l])
        for j in missed:
            patch_port.append(i)
            patch_date.append(int(j))
    plan["patch_port"] = np.array(patch_port, dtype=np.int64)
    plan["patch_date"] = np.array(patch_date, dtype=np.int32)
    return plan


def backtest_portfolios_grid(portfolio_specs_list, ts_start_date, ts_end_date, market_data, turnover_costs=None):
    """`backtest_portfolio` for ONE grid family - the specs `calculate_weights_for_grid` accepts, all of one rebalancing
    frequency - with the weights never leaving the device: the pack, the upload and the grid sweep of
    `calculate_weights_for_grid` (`_grid_sweep_stage`, weights not downloaded), then ONE `Batch.replay` of all specs that reads
    the sweep's results where they lie; only statuses, P&L, turnover and metrics cross to the host.  Per spec, as there: the
    statuses of the served entries are checked (`_raise_on_status`), the dates the pack does not serve and the specs whose size
    is outside the sweep are solved by `_weights_for_dates` and go up as patch rows with that spec's own copy of the universe
    rows; different risk aversions become a per-spec scale 1.0 / risk_aversion on the device, the host's `1.0 / g * w`.
    Returns {display_name: dict}, the dicts of `_replay_backtest` - equal bit for bit to `calculate_weights_for_grid` followed by
    `replay_backtests_device`.  "Weights do not sum to 1." raises the reference's ValueError.  Without a sweep that serves the
    family (a pack that raises, no size within the sweep) it is exactly that pair of calls.
    Opt-in: nothing calls it by default.  It does not fill the spec caches `calculate_weights_for_grid` fills: the weights are
    never on the host.
    `turnover_costs` (basis points): instead of the dicts, the metrics table of `summarise_backtests_device` for the family at
    every one of these costs - the replay runs once at cost 0 and keeps its results on the device (`download=False`), so only
    statuses and 256 bytes per (spec, cost) come down; the specs' own `turnover_cost` is not read."""
    specs = list(portfolio_specs_list)
    if not specs:
        return {}
    trading_dates = [pd.Timestamp(ts) for ts in market_data["stock_prices_df"].index]
    trading_dates = [ts for ts in trading_dates if ts_start_date <= ts <= ts_end_date]
    rebalance_dates = rebalancing_schedule(trading_dates, specs[0]["rebalancing_frequency"])
    tickers = batch.panels_for(market_data, specs[0]["rolling_window_frequency"]).tickers
    sizes, windows, conj, same_gamma, swept, b = _grid_sweep_stage(rebalance_dates, specs, market_data, want_weights=False,
                                                                   keep_open=True)
    try:
        R = len(rebalance_dates)
        fits = swept is not None and any(int(sp["size"]) in sizes for sp in specs)
        if fits:
            _none, status, labels, cols, caps, mask, prior_keys = swept
            k = sizes[-1]
            # (an unswept spec reads no source row, but its k rows at offset 0 must lie inside the source all the same)
            fits = max(int(sp["size"]) for sp in specs) <= status.size * k
        if not fits:
            if b is not None:
                b.close()
                b = None
            found = calculate_weights_for_grid(rebalance_dates, specs, market_data)
            items = [(res[0], res[2], res[3], sp) for res, sp in zip(found, specs)]
            if turnover_costs is not None:
                return summarise_backtests_device(trading_dates, rebalance_dates, items, market_data, turnover_costs, tickers=tickers)
            results = replay_backtests_device(trading_dates, rebalance_dates, items, market_data, tickers=tickers)
            return {sp["display_name"]: res for sp, res in zip(specs, results)}
        plan = _grid_replay_plan(specs, sizes, windows, prior_keys, mask, k)
        # universe tables: the pack's [R x k] first (a served spec holds its prefix, stride k); a patched spec's own copy after it
        c_parts, p_parts = [np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)], [np.ascontiguousarray(caps, dtype=np.float64).reshape(-1)]
        u_len = R * k
        u_off, u_stride, rows = [], [], []
        for i, sp in enumerate(specs):
            ks = int(sp["size"])
            miss = plan["patch_date"][plan["patch_port"] == i]
            if plan["swept"][i]:
                served = mask[:, sizes.index(ks), windows.index(int(sp["rolling_window"]))]
                _raise_on_status(status.reshape(R, -1)[served, plan["s_off"][i]])
            if not miss.size:
                u_off.append(0)
                u_stride.append(k)
                continue
            alone = _weights_for_dates([rebalance_dates[j] for j in miss], sp, market_data)
            if plan["swept"][i]:
                own_cols, own_caps = cols[:, :ks].copy(), caps[:, :ks].copy()
            else:
                own_cols, own_caps = np.empty((R, ks), dtype=np.int32), np.empty((R, ks), dtype=np.float64)
            for q, j in enumerate(miss):
                own_cols[j], own_caps[j] = alone[2][q], alone[3][q]
                rows.append(np.asarray(alone[0][q], dtype=np.float64))
            u_off.append(u_len)
            u_stride.append(ks)
            c_parts.append(np.ascontiguousarray(own_cols, dtype=np.int32).reshape(-1))
            p_parts.append(np.ascontiguousarray(own_caps, dtype=np.float64).reshape(-1))
            u_len += R * ks
        patches = None
        if rows:
            patch_rows = np.zeros((len(rows), max(r.size for r in rows)), dtype=np.float64)
            for q, r in enumerate(rows):
                patch_rows[q, :r.size] = r
            patches = (plan["patch_port"], plan["patch_date"], patch_rows)
        S, rf_daily, reb_day = _device_replay_inputs(trading_dates, rebalance_dates, market_data, tickers)
        table = None
        replayed = b.replay(
            _native.REPLAY_SRC_GRID_SWEEP, S, rf_daily, reb_day, len(tickers), np.array([int(sp["size"]) for sp in specs], dtype=np.int32),
            np.array([sp["risk_aversion"] if sp.get("risk_aversion") is not None else 1 for sp in specs], dtype=np.float64),
            np.array([sp["turnover_cost"] if turnover_costs is None else 0.0 for sp in specs], dtype=np.float64),
            plan["w_off"], plan["w_stride"], plan["s_off"], plan["s_stride"], np.array(u_off, dtype=np.int64),
            np.array(u_stride, dtype=np.int64), np.concatenate(c_parts), np.concatenate(p_parts),
            w_scale=plan["w_scale"], patches=patches, download=turnover_costs is None)
        if turnover_costs is not None:
            table = _summary_table(b.dev, trading_dates, specs, market_data, turnover_costs)
            if table is None:                                     # a replay status: which one decides what is raised, below
                replayed = b.dev._replay_download(len(specs), len(trading_dates), R)
        returns, turnover, metrics, rstatus, _bad_day = replayed if replayed is not None else (None, None, None, 0, None)
    finally:
        if b is not None:
            b.close()
    rstatus = np.asarray(rstatus)
    if np.any(rstatus == _native.REPLAY_BAD_WEIGHTS):
        raise RuntimeError("backtest_portfolios_grid: the replay read a weight row its sweep flagged, although every served status "
                           "was checked")
    if np.any(rstatus != 0):
        logger.error("Weights do not sum to 1.")
        raise ValueError("Weights do not sum to 1.")
    if table is not None:
        return table
    results = _device_replay_results(trading_dates, rebalance_dates, specs, returns, turnover, metrics)
    return {sp["display_name"]: res for sp, res in zip(specs, results)}


def backtest_portfolio(portfolio_spec, ts_start_date, ts_end_date, market_data):
    """Same inputs and outputs as ref:1221-1238.  All posterior solves of the backtest happen in ONE device
    batch, and the daily replay runs over arrays (`_replay_backtest`); `Portfolio.update_portfolio` remains the
    day-at-a-time form of the same loop."""
    trading_dates = [pd.Timestamp(ts) for ts in market_data["stock_prices_df"].index]
    trading_dates = [ts for ts in trading_dates if ts_start_date <= ts <= ts_end_date]
    rebalance_dates = rebalancing_schedule(trading_dates, portfolio_spec["rebalancing_frequency"])
    _prefetch_siblings(portfolio_spec, rebalance_dates, market_data)
    weights, labels, cols, caps = _weights_for_dates(rebalance_dates, portfolio_spec, market_data)
    tickers = batch.panels_for(market_data, portfolio_spec["rolling_window_frequency"]).tickers
    return _replay_backtest(trading_dates, rebalance_dates, weights, cols, caps, tickers, portfolio_spec, market_data)


def backtest_portfolio_device(portfolio_spec, ts_start_date, ts_end_date, market_data, turnover_costs=None):
    """`backtest_portfolio` for a `greyserman` or `jorion` spec with the weights never leaving the device: the pack of
    `_weights_for_dates`, ONE batch, its solve sweep (the draws' ridge shifts, or Jorion's single solve; right-hand sides [t, 1]),
    `Batch.sweep_finish` with the spec's risk aversion, then `Batch.replay(REPLAY_SRC_SWEEP_FINISH, ...)` reads the [W x k]
    weights where the finish wrote them (no scale: the finish has divided by gamma).  A `greyserman` spec with
    GREYSERMAN_SPECTRAL set, up to `sweep_max_assets()`: `Batch.spectral_greyserman` in place of the sweep and the finish, read
    through REPLAY_SRC_SPECTRAL, whatever the number of dates.  Returns the dict of `_replay_backtest` -
    equal bit for bit to `_weights_for_dates` with the device finish switched on followed by `replay_backtests_device` - or, with
    `turnover_costs` (basis points), the metrics table of `summarise_backtests_device` for the spec at every one of these costs
    (the replay runs at cost 0 and keeps its results on the device).  A date the finish flagged raises what `_raise_on_status`
    raises; "Weights do not sum to 1." raises the reference's ValueError.
    When the dates do not fit one sweep's solution budget (_GREYSERMAN_SWEEP_BYTES), or a Greyserman universe above
    `sweep_max_assets()` without GREYSERMAN_TILED_SWEEP, it is `_weights_for_dates` + `replay_backtests_device` (or
    `summarise_backtests_device`).  Opt-in: nothing calls it by default."""
    strategy = portfolio_spec["weighting_strategy"]
    if strategy not in ("greyserman", "jorion"):
        raise ValueError(f"backtest_portfolio_device serves greyserman and jorion specs, not {strategy!r}")
    grey = strategy == "greyserman"
    trading_dates = [pd.Timestamp(ts) for ts in market_data["stock_prices_df"].index]
    trading_dates = [ts for ts in trading_dates if ts_start_date <= ts <= ts_end_date]
    rebalance_dates = rebalancing_schedule(trading_dates, portfolio_spec["rebalancing_frequency"])
    tickers = batch.panels_for(market_data, portfolio_spec["rolling_window_frequency"]).tickers
    k, N, gamma = portfolio_spec["size"], portfolio_spec["rolling_window"], portfolio_spec["risk_aversion"]
    W = len(rebalance_dates)
    B = GREYSERMAN_DRAWS if grey else 1
    fits = W * B * 2 * k * 8 <= _GREYSERMAN_SWEEP_BYTES
    if grey and k > _native.sweep_max_assets() and not GREYSERMAN_TILED_SWEEP:
        fits = False
    spectral = grey and GREYSERMAN_SPECTRAL and k <= _native.sweep_max_assets()
    if spectral:
        fits = True                                           # (the spectral sweep keeps no solutions: no budget to fit)
    source = _native.REPLAY_SRC_SPECTRAL if spectral else _native.REPLAY_SRC_SWEEP_FINISH
    if not fits:
        weights, _labels, cols, caps = _weights_for_dates(rebalance_dates, portfolio_spec, market_data)
        items = [(weights, cols, caps, portfolio_spec)]
        if turnover_costs is not None:
            return summarise_backtests_device(trading_dates, rebalance_dates, items, market_data, turnover_costs, tickers=tickers)
        return replay_backtests_device(trading_dates, rebalance_dates, items, market_data, tickers=tickers)[0]
    kw, _labels, caps = batch.pack_windows(list(rebalance_dates), portfolio_spec, market_data,
                                           members_of=_members_provider(market_data), return_caps=True)
    cols = kw["col_idx"]
    n_rows = np.asarray(kw["n_rows"])
    if not grey:
        kw.pop("start", None)                                 # (as `_weights_for_dates` hands a Jorion pack on)
    flags = _native.FLAG_NO_CENTER if grey else _native.FLAG_CENTER_BY_ROWS
    b = _native.Batch(_native.default_device(), "jeffreys", k, N, kw["n_r"], 1.0, W, 0, flags=flags)
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        if spectral:
            xi, eta = _greyserman_hyper(W, None)
            b.spectral_greyserman(n_rows.astype(np.float64), gamma, _greyserman_kappa(n_rows), xi, eta)
        elif grey:
            xi, eta = _greyserman_hyper(W, None)
            shift = np.zeros((W, B, 2))
            shift[:, :, 0] = eta / 2
            _finish_sweep(b, k, shift).sweep_finish(_native.FINISH_GREYSERMAN, n_rows.astype(np.float64), gamma,
                                                    kappa=_greyserman_kappa(n_rows), xi=xi, eta=eta)
        else:
            _finish_sweep(b, k, None).sweep_finish(_native.FINISH_JORION, n_rows.astype(np.float64), gamma)
        S, rf_daily, reb_day = _device_replay_inputs(trading_dates, rebalance_dates, market_data, tickers)
        one = lambda v, dtype: np.array([v], dtype=dtype)     # noqa: E731
        table = None
        replayed = b.replay(
            source, S, rf_daily, reb_day, len(tickers), one(k, np.int32),
            one(gamma if gamma is not None else 1, np.float64),
            one(portfolio_spec["turnover_cost"] if turnover_costs is None else 0.0, np.float64),
            one(0, np.int64), one(k, np.int64), one(0, np.int64), one(1, np.int64), one(0, np.int64), one(k, np.int64),
            np.ascontiguousarray(cols, dtype=np.int32).reshape(-1), np.ascontiguousarray(caps, dtype=np.float64).reshape(-1),
            w_scale=None, download=turnover_costs is None)
        if turnover_costs is not None:
            table = _summary_table(b.dev, trading_dates, [portfolio_spec], market_data, turnover_costs)
            if table is None:                                     # a replay status: which one decides what is raised, below
                replayed = b.dev._replay_download(1, len(trading_dates), W)
        returns, turnover, metrics, rstatus, _bad_day = replayed if replayed is not None else (None, None, None, 0, None)
        if np.any(np.asarray(rstatus) == _native.REPLAY_BAD_WEIGHTS):
            if spectral:
                _raise_on_spectral_status(b.download_spectral()[1])
            else:
                _raise_on_status(b.download_sweep_finish()[1])
            raise RuntimeError("backtest_portfolio_device: the replay read a weight row the finish flagged with an unknown status")
    finally:
        b.close()
    if np.any(np.asarray(rstatus) != 0):
        logger.error("Weights do not sum to 1.")
        raise ValueError("Weights do not sum to 1.")
    if table is not None:
        return table
    return _device_replay_results(trading_dates, rebalance_dates, [portfolio_spec], returns, turnover, metrics)[0]


def backtest_portfolios(portfolio_specs_dict, ts_start_date, ts_end_date, market_data):
    """`backtest_portfolio` for a whole spec grid ({name: spec}, as `create_portfolio_specs` returns it): the
    conjugate specs that share their windows go to the device in ONE batch (`calculate_weights_for_specs`), then
    every spec is replayed.  Specs outside the scope of this build (shrinkage, Black-Litterman: pypfopt) are
    skipped with a warning unless the caller supplied them (`register_strategy`)."""
    trading_dates = [pd.Timestamp(ts) for ts in market_data["stock_prices_df"].index]
    trading_dates = [ts for ts in trading_dates if ts_start_date <= ts <= ts_end_date]
    groups = {}
    for name, sp in portfolio_specs_dict.items():
        if sp["weighting_strategy"] in _CONJUGATE:
            groups.setdefault(_batch_family(sp), []).append(sp)
    for family, specs in groups.items():
        if len(specs) > 1:
            calculate_weights_for_specs(rebalancing_schedule(trading_dates, specs[0]["rebalancing_frequency"]), specs, market_data)
    out = {}
    pending = {}          # DEVICE_REPLAY: (rebalancing frequency, ticker list) -> [(name, weights, cols, caps, spec)]
    for name, sp in portfolio_specs_dict.items():
        if sp["weighting_strategy"] in _OUT_OF_SCOPE and sp["weighting_strategy"] not in _EXTERNAL_STRATEGIES:
            logger.warning(f"{name}: {sp['weighting_strategy']} is outside the scope of this build (pypfopt); skipped.")
            continue
        if not DEVICE_REPLAY:
            out[name] = backtest_portfolio(sp, ts_start_date, ts_end_date, market_data)
            continue
        # every spec's weights as `backtest_portfolio` obtains them; the replay waits for the whole group
        rebalance_dates = rebalancing_schedule(trading_dates, sp["rebalancing_frequency"])
        _prefetch_siblings(sp, rebalance_dates, market_data)
        weights, labels, cols, caps = _weights_for_dates(rebalance_dates, sp, market_data)
        tickers = batch.panels_for(market_data, sp["rolling_window_frequency"]).tickers
        out[name] = None                                                  # (keeps the specs' order)
        pending.setdefault((sp["rebalancing_frequency"], tuple(tickers)), []).append((name, weights, cols, caps, sp))
    for (frequency, tickers), members in pending.items():
        results = replay_backtests_device(trading_dates, rebalancing_schedule(trading_dates, frequency),
                                          [m[1:] for m in members], market_data, tickers=list(tickers))
        for m, res in zip(members, results):
            out[m[0]] = res
    return out
