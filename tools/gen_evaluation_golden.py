#!/usr/bin/env python3
"""Writes tests/golden/evaluation_helpers.npz: inputs and outputs of the three helpers of the reference's evaluation that run
without QuantStats - adjust_returns, get_insolvent_date, compute_excess_returns - for tests/test_host_replay_summary.py.

    python tools/gen_evaluation_golden.py REFERENCE_SRC_DIR

REFERENCE_SRC_DIR holds the reference's portfolio_evaluation.py.  The module is imported unmodified; the plotting, QuantStats
and dotenv modules it imports at the top and that may be absent are stubbed in sys.modules (none of the three helpers touches
them).  The tests read the .npz, never the reference."""
import importlib
import os
import sys
import types

import numpy as np
import pandas as pd

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "evaluation_helpers.npz")
STUBS = ("quantstats", "dotenv", "matplotlib", "matplotlib.pyplot", "matplotlib.dates", "matplotlib.ticker", "seaborn",
         "portfolio_specs")


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        return lambda *a, **k: None


def _series():
    rng = np.random.default_rng(20240611)
    quiet = rng.normal(0.0005, 0.01, 12)
    cases = {"none": quiet.copy()}
    cases["first_day"] = np.concatenate([[-2.5], quiet[:7]])
    mid = quiet.copy()
    mid[5] = -2.5
    cases["mid_series"] = mid
    cases["zero_prev_cum_return"] = np.array([0.0, 0.0, -2.5, 0.01, 0.02])
    before = quiet.copy()
    before[2], before[7] = -0.995, -3.0
    cases["insolvent_before_adjusted"] = before
    only = quiet.copy()
    only[4] = -0.995
    cases["insolvent_not_adjusted"] = only
    down = np.abs(quiet) + 0.001
    down[6] = -1.75
    cases["adjusted_from_above_one"] = down
    return cases


def main(src_dir):
    sys.path.insert(0, src_dir)
    for name in STUBS:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
    ref = importlib.import_module("portfolio_evaluation")
    out = {}
    with np.errstate(all="ignore"):
        for name, values in _series().items():
            s = pd.Series(values, index=pd.bdate_range("2022-03-01", periods=values.size), name=name)
            adjusted = ref.adjust_returns(s)
            day = lambda ts: -1 if ts is None else int(s.index.get_loc(ts))   # noqa: E731
            out[f"{name}/in"] = values
            out[f"{name}/adjusted"] = adjusted.to_numpy(dtype=np.float64)
            out[f"{name}/insolvent_raw"] = np.int64(day(ref.get_insolvent_date(s)))
            out[f"{name}/insolvent_adjusted"] = np.int64(day(ref.get_insolvent_date(adjusted)))
    # DTB3 quoted on some days only, with gaps at both ends of the portfolio's days
    days = pd.bdate_range("2022-03-01", periods=15)
    quoted = days[[3, 4, 7, 11]]
    rates = pd.DataFrame({"DTB3": [0.011, np.nan, 0.013, 0.017]}, index=quoted)
    returns = pd.Series(np.random.default_rng(7).normal(0.0, 0.01, days.size), index=days, name="p")
    excess = ref.compute_excess_returns(returns, rates)
    out["excess/days"] = days.values.astype("datetime64[ns]").astype(np.int64)
    out["excess/returns"] = returns.to_numpy()
    out["excess/quoted"] = quoted.values.astype("datetime64[ns]").astype(np.int64)
    out["excess/rates"] = rates["DTB3"].to_numpy()
    out["excess/out"] = excess.to_numpy(dtype=np.float64)
    np.savez(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
