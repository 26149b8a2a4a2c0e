"""The replay summary without a GPU: the restated helpers of the reference's evaluation against values the reference itself
produced (tests/golden/evaluation_helpers.npz, written by tools/gen_evaluation_golden.py), the host yardstick
`summary_records_host` against the long-double truth of tests/_replay_summary_reference.py at a quarter of the tolerance (the
device gets the whole, tests/test_gpu_replay_summary.py), `performance_table` against the reference's own CHECK formulas and
scipy, and the margin condition every case must meet."""
import os

import numpy as np
import pandas as pd
import pytest
from scipy.stats import kurtosis, norm, skew

from incorporating_different_sources_amd import _native, portfolio_evaluation as pe

import _replay_summary_reference as ref

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "evaluation_helpers.npz"))
SERIES = sorted({name.split("/")[0] for name in GOLDEN.files} - {"excess"})


def test_the_golden_inputs_cover_what_they_must():
    day = {name: (int(GOLDEN[f"{name}/insolvent_adjusted"]),
                  int(np.flatnonzero(GOLDEN[f"{name}/in"] != GOLDEN[f"{name}/adjusted"])[0]) if
                  (GOLDEN[f"{name}/in"] != GOLDEN[f"{name}/adjusted"]).any() else -1) for name in SERIES}
    assert day["none"] == (-1, -1)
    assert day["first_day"][1] == 0 and day["mid_series"][1] > 0
    assert np.isinf(GOLDEN["zero_prev_cum_return/adjusted"]).any()
    ins, adj = day["insolvent_before_adjusted"]
    assert 0 <= ins < adj
    assert day["mid_series"][0] == day["mid_series"][1]                      # insolvent on the adjusted day
    assert day["insolvent_not_adjusted"][0] >= 0 and day["insolvent_not_adjusted"][1] == -1
    rates, quoted, days = GOLDEN["excess/rates"], GOLDEN["excess/quoted"], GOLDEN["excess/days"]
    assert np.isnan(rates).any() and days[0] < quoted[0] and quoted[-1] < days[-1]


@pytest.mark.parametrize("name", SERIES)
def test_adjust_returns_and_get_insolvent_date_against_the_reference(name):
    values, want = GOLDEN[f"{name}/in"], GOLDEN[f"{name}/adjusted"]
    s = pd.Series(values, index=pd.bdate_range("2022-03-01", periods=values.size))
    got = pe.adjust_returns(s)
    assert got.index.equals(s.index)
    got = got.to_numpy()
    changed = values != want
    assert np.array_equal(got[~changed], want[~changed])                     # unadjusted values and the zeros: exact
    if changed.any():
        i = int(np.flatnonzero(changed)[0])
        assert got[i] == want[i] if np.isinf(want[i]) else abs(got[i] - want[i]) <= 1e-12 * abs(want[i])
        assert (got[i + 1:] == 0).all()
    for kind, series in (("raw", s), ("adjusted", pd.Series(want, index=s.index))):
        ts = pe.get_insolvent_date(series)
        assert (-1 if ts is None else s.index.get_loc(ts)) == int(GOLDEN[f"{name}/insolvent_{kind}"])
    # the array form the records are built from agrees with the Series form
    arr, at = pe._adjust(values)
    assert np.array_equal(arr, got, equal_nan=True) and at == (int(np.flatnonzero(changed)[0]) if changed.any() else -1)


def test_compute_excess_returns_against_the_reference():
    days = pd.DatetimeIndex(GOLDEN["excess/days"].astype("datetime64[ns]"))
    rates = pd.DataFrame({"DTB3": GOLDEN["excess/rates"]}, index=pd.DatetimeIndex(GOLDEN["excess/quoted"].astype("datetime64[ns]")))
    returns = pd.Series(GOLDEN["excess/returns"], index=days, name="p")
    got = pe.compute_excess_returns(returns, rates)
    assert got.name == "p" and got.index.equals(days)
    assert np.array_equal(got.to_numpy(), GOLDEN["excess/out"])
    # rf_excess_for: what the device subtracts on days[1:] is what the reference subtracts from a series dated days[1:]
    rf = pe.rf_excess_for(days, rates)
    want = returns.iloc[1:] - pe.compute_excess_returns(returns.iloc[1:], rates)
    assert np.isnan(rf[0]) and np.allclose(rf[1:], want.to_numpy(), rtol=0, atol=1e-18)


@pytest.mark.parametrize("name", ref.CASES)
def test_every_case_meets_the_margin_condition_and_shows_what_it_is_for(name):
    ref.check_case(ref.case(name), ref.host_case(name)[2])


@pytest.mark.parametrize("name", ref.CASES)
def test_host_records_against_the_truth_at_a_quarter_of_the_tolerance(name):
    c = ref.case(name)
    ret, turn, truth = ref.host_case(name)
    stats, status = pe.summary_records_host(ret, turn, c.call["reb_day"], c.cost_bp, c.rf_excess)
    worst = ref.ratio(stats, status, truth, name)
    print(f"{name}: host / tolerance = {worst:.3g}")
    assert worst <= 0.25
    if (truth.stats[..., ref.ADJ_DAY] < 0).all():                           # selections: bit-equal without an adjusted day
        for f in (ref.BEST, ref.WORST):
            assert np.array_equal(stats[..., f], truth.stats[..., f].astype(np.float64), equal_nan=True)


def test_no_turnover_reaches_a_day_that_is_not_a_rebalancing_day():
    """A NaN turnover on date 2 reaches day reb_day[2] at every cost, 0 included (0 x NaN), and no other day; a replay status
    gives a NaN record and leaves the neighbours alone."""
    rng = np.random.default_rng(5)
    D, reb = 40, np.array([0, 10, 20, 30])
    ret = np.full((3, D), np.nan)
    ret[:, 1:] = rng.normal(0.0, 0.01, (3, D - 1))
    turn = np.full((3, 4), np.nan)
    turn[:, 1:] = 0.4
    rf = np.full(D, 1e-4)
    clean, clean_status = pe.summary_records_host(ret, turn, reb, [0.0, 15.0], rf)
    assert (clean_status == pe.SUMMARY_OK).all()
    turn[1, 2] = np.nan
    stats, status = pe.summary_records_host(ret, turn, reb, [0.0, 15.0], rf, replay_status=[0, 0, 1])
    assert status.tolist() == [[0, 0], [pe.SUMMARY_NONFINITE] * 2, [pe.SUMMARY_NO_REPLAY] * 2]
    assert stats[0].tobytes() == clean[0].tobytes()
    assert np.isnan(stats[2, :, :28]).all() and (stats[2, :, 28:] == 0).all()
    kept = list(pe.KEPT_WHEN_NONFINITE)
    assert np.array_equal(stats[1][:, kept], clean[1][:, kept])
    assert np.isnan(np.delete(stats[1], kept + [28, 29, 30, 31], axis=1)).all()
    x, _e = ref.net_and_excess(ret[1], turn[1], reb, 15.0, rf)
    assert np.flatnonzero(np.isnan(x)).tolist() == [19]                      # day 20 alone


def test_performance_table_against_the_check_formulas_and_scipy():
    name = "D700-monthly-P37-C5"
    c = ref.case(name)
    ret, turn, _truth = ref.host_case(name)
    stats, status = pe.summary_records_host(ret, turn, c.call["reb_day"], c.cost_bp, c.rf_excess)
    days = pd.bdate_range("2019-01-02", periods=ret.shape[1])
    bench = np.random.default_rng(3).normal(0.0003, 0.01, ret.shape[1] - 1)
    names = [f"p{p}" for p in range(ret.shape[0])]
    table = pe.performance_table(stats, status, days, names, c.cost_bp, benchmark_excess=bench)
    assert list(table.columns) == pe.METRICS and table.index.names == ["name", "turnover_cost"]
    assert len(table) == ret.shape[0] * c.cost_bp.size
    for p, ci in ((0, 0), (5, 2), (36, 4)):
        x, e = ref.net_and_excess(ret[p], turn[p], c.call["reb_day"], c.cost_bp[ci], c.rf_excess)
        s, es = pd.Series(x, index=days[1:]), pd.Series(e, index=days[1:])
        row = table.loc[(names[p], c.cost_bp[ci])].astype(float)
        close = lambda a, b: abs(a - b) <= 1e-9 * max(1.0, abs(b))              # noqa: E731
        assert close(row["Cum. Return"], (1 + s).prod() - 1)
        assert close(row["CAGR"], ((1 + s).prod()) ** (1 / ((s.index[-1] - s.index[0]).days / 365)) - 1)           # ref:524
        assert close(row["Sharpe"], es.mean() / es.std() * (252 ** 0.5))                                          # ref:541
        assert close(row["Avg. Loss"], s[s < -1e-7].mean())                                                       # ref:592
        assert close(row["Avg. Return"], s.mean())                                                                # ref:607
        assert close(row["Avg. Win"], s[s > 1e-7].mean())                                                         # ref:623
        assert close(row["Ann. Vol."], s.std() * 252 ** 0.5)                                                      # ref:655
        assert close(row["Best Day"], s.max()) and close(row["Worst Day"], s.min())
        assert close(row["Daily VaR"], norm.ppf(0.05, s.mean(), s.std()))
        wealth = (1 + s).cumprod()
        assert close(row["Max. DD"], (wealth / wealth.cummax() - 1).min())
        assert close(row["Calmar"], row["CAGR"] / abs(row["Max. DD"]))
        assert close(row["Sortino"], es.mean() / np.sqrt((es[es < 0] ** 2).sum() / es.size) * 252 ** 0.5)
        assert close(row["Avg. Turnover"], np.mean(turn[p, 1:]))
        sr, bsr = es.mean() / es.std(), bench.mean() / bench.std(ddof=1)                                           # ref:86-118
        sigma = np.sqrt((1 - skew(es) * sr + (kurtosis(es, fisher=False) - 1) / 4 * sr ** 2) / (es.size - 1))
        assert close(row["Prob. Sharpe"], norm.cdf((sr - bsr) / sigma))
    assert np.isnan(pe.performance_table(stats, status, days, names, c.cost_bp)["Prob. Sharpe"].astype(float)).all()


def test_performance_table_of_an_insolvent_portfolio_and_of_a_refused_record():
    name = "insolvent-before-adjust"
    c = ref.case(name)
    ret, turn, truth = ref.host_case(name)
    stats, status = pe.summary_records_host(ret, turn, c.call["reb_day"], c.cost_bp, c.rf_excess, replay_status=[0, 1, 0, 0, 0])
    days = pd.bdate_range("2019-01-02", periods=ret.shape[1])
    table = pe.performance_table(stats, status, days, list("abcde"), c.cost_bp)
    row = table.loc[("a", 15.0)]
    assert all(row[m] is None for m in pe.NONE_WHEN_INSOLVENT)                                                    # ref:520-576
    x, _e = ref.net_and_excess(ret[0], turn[0], c.call["reb_day"], 15.0, c.rf_excess)
    a = pe._adjust(x)[0]
    assert abs(row["Avg. Return"] - a[np.abs(a) > 1e-7].mean()) < 1e-12                                           # ref:612
    assert abs(row["Worst Day"] - a[:29].min()) < 1e-15 and abs(row["Ann. Vol."] - np.std(a[:29], ddof=1) * 252 ** 0.5) < 1e-12
    assert abs(row["Avg. Turnover"] - turn[0, 1:2].mean()) < 1e-15                # dates up to day 30: day 21 alone (ref:696)
    assert table.loc["b"].isna().all().all()


def test_exports_list_the_summary():
    for sym in ("tp_replay_summary", "tp_replay_download_summary"):
        assert sym in _native.EXPORTS and hasattr(_native.lib, sym)
    assert _native.SUMMARY_STATS == pe.SUMMARY_STATS == ref.NSTATS
    assert _native.lib.tp_replay_summary(None, 1, None, None) == _native.TP_ERR_INVALID
    assert _native.lib.tp_replay_download_summary(None, None, None) == _native.TP_ERR_INVALID
