"""Size sweep, what can be checked without a GPU: the C-ABI symbols, the binding's argument checks (before any device call),
the host mask of batch.pack_windows_nested, the nesting of select_universe, and that calculate_weights_for_specs keeps refusing
mixed sizes."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import REPO
from incorporating_different_sources_amd import _native, batch, synthetic

SYMBOLS = ("tp_batch_size_sweep", "tp_batch_download_size_sweep")
N = 30
SIZES = [4, 8, 12]


def test_size_sweep_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "tangency_posterior.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", code), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"libtangency.so does not export {name}"
        assert name in _native.EXPORTS


class _NoDevice:
    """Stands in for the device and the library handle: any call into the library fails the test."""
    def _check(self, rc):
        pytest.fail("the binding called into the library")


def _batch(W=3, k=6):
    b = object.__new__(_native.Batch)
    b.dev, b.W, b.k, b._b = _NoDevice(), W, k, ctypes.c_void_p()
    return b


@pytest.mark.parametrize("sizes,n0,w0", [
    ([], np.ones((3, 2)), np.ones((3, 2, 0, 6))),                      # no size
    (list(range(1, 18)), None, None),                                  # more than 16 sizes
    ([0, 3], np.ones((3, 2)), np.ones((3, 2, 2, 6))),                  # below 1
    ([3, 7], np.ones((3, 2)), np.ones((3, 2, 2, 6))),                  # above k
    ([3, 3], np.ones((3, 2)), np.ones((3, 2, 2, 6))),                  # not strictly increasing
    ([4, 2], np.ones((3, 2)), np.ones((3, 2, 2, 6))),
    ([[2, 4]], np.ones((3, 2)), np.ones((3, 2, 2, 6))),                # not 1-D
    ([2.0, 4.0], np.ones((3, 2)), np.ones((3, 2, 2, 6))),              # not integers
    (None, np.ones((3, 2)), np.ones((3, 2, 2, 6))),
    ([2, 4], np.ones((3,)), np.ones((3, 1, 2, 6))),                    # n0 not [W x P]
    ([2, 4], np.ones((2, 2)), np.ones((2, 2, 2, 6))),                  # wrong W
    ([2, 4], np.ones((3, 0)), np.ones((3, 0, 2, 6))),                  # P = 0
    ([2, 4], np.ones((3, 2)), np.ones((3, 2, 2, 5))),                  # wrong k
    ([2, 4], np.ones((3, 2)), np.ones((3, 2, 3, 6))),                  # S of w0 differs
    ([2, 4], np.ones((3, 2)), np.ones((3, 2, 6))),                     # w0 not 4-D
    ([2, 4], np.ones((3, 2), dtype=complex), np.ones((3, 2, 2, 6))),   # dtypes that are not real numbers
    ([2, 4], np.ones((3, 2)), np.full((3, 2, 2, 6), "x")),
    ([2, 4], None, np.ones((3, 2, 2, 6))),                             # one of the two priors alone
    ([2, 4], np.ones((3, 2)), None),
])
def test_binding_rejects_wrong_shapes_dtypes_and_size_lists_before_any_device_call(sizes, n0, w0, monkeypatch):
    monkeypatch.setattr(_native.lib, "tp_batch_size_sweep", lambda *a: pytest.fail("the binding called into the library"), raising=False)
    with pytest.raises(ValueError):
        _batch().size_sweep(sizes, n0, w0)


def _spec(strat="conjugate_hf_vix_vw", k=12):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": "daily",
            "rolling_window": N, "rolling_window_frequency": "daily", "mcm_scaling": 1, "display_name": strat}


def _market(n_tickers=16):
    md, _ = synthetic.make_market_data(n_tickers=n_tickers, n_days=N + 30, seed=20240092)
    days = md["stock_prices_df"].index
    return md, [pd.Timestamp(d) for d in days[N + 5:N + 11]]


def _plant_intraday_nan(md, date, ticker, bar=40):
    hf = md["stock_intraday_prices_df"].copy()
    rows = np.flatnonzero(hf.index.normalize() == date)
    hf.iloc[rows[bar], hf.columns.get_loc(ticker)] = np.nan
    return dict(md, stock_intraday_prices_df=hf)


def test_nested_pack_mask_follows_the_rows_the_smaller_universe_would_keep():
    """A NaN bar of the SMALLEST-cap selected stock drops intraday rows from the pack that the universes without that stock
    keep: at that date those sizes cannot be served from the pack (the largest size is the pack itself).  The same NaN in the
    LARGEST-cap stock drops the same rows at every size: every mask is true."""
    md, dates = _market()
    batch.clear_panel_cache()
    kw, labels, caps, mask = batch.pack_windows_nested(dates, _spec(), SIZES, md)
    assert mask.shape == (len(dates), len(SIZES)) and mask.all()
    assert kw["col_idx"].shape == (len(dates), SIZES[-1]) and caps.shape == (len(dates), SIZES[-1])
    assert (np.diff(caps, axis=1) <= 0).all()                          # cap-descending: the prefixes are the larger caps
    plain = batch.pack_windows(dates, _spec(), md, return_caps=True)
    assert np.array_equal(plain[0]["col_idx"], kw["col_idx"]) and plain[1] == labels and np.array_equal(plain[2], caps)
    w = 2
    batch.clear_panel_cache()
    kw2, _, _, mask2 = batch.pack_windows_nested(dates, _spec(), SIZES, _plant_intraday_nan(md, dates[w], labels[w][-1]), None)
    expect = np.ones_like(mask)
    expect[w, :-1] = False
    assert np.array_equal(mask2, expect), mask2
    assert kw2["hf_count"][w] < kw["hf_count"][w] and np.array_equal(np.delete(kw2["hf_count"], w), np.delete(kw["hf_count"], w))
    # a stock inside the 8 largest but not the 4 largest: size 4 alone loses the prefix's rows
    batch.clear_panel_cache()
    mask3 = batch.pack_windows_nested(dates, _spec(), SIZES, _plant_intraday_nan(md, dates[w], labels[w][5]))[3]
    expect = np.ones_like(mask)
    expect[w, 0] = False
    assert np.array_equal(mask3, expect), mask3
    batch.clear_panel_cache()
    mask4 = batch.pack_windows_nested(dates, _spec(), SIZES, _plant_intraday_nan(md, dates[w], labels[w][0]))[3]
    assert mask4.all()
    batch.clear_panel_cache()


def test_nested_pack_raises_when_a_date_has_fewer_eligible_stocks_than_the_largest_size():
    md, dates = _market(n_tickers=12)
    caps = md["stock_market_caps_df"].copy()
    caps.loc[dates[3], caps.columns[:2]] = np.nan                      # 10 stocks with a cap at that date
    batch.clear_panel_cache()
    with pytest.raises(ValueError):
        batch.pack_windows_nested(dates, _spec(), SIZES, dict(md, stock_market_caps_df=caps))
    batch.clear_panel_cache()
    with pytest.raises(ValueError):
        batch.pack_windows_nested(dates, _spec(), [8, 4], md)          # sizes must increase
    batch.clear_panel_cache()


def test_select_universe_is_nested_in_size():
    md, dates = _market()
    batch.clear_panel_cache()
    mp = batch.panels_for(md, "daily")
    members = np.ones(len(mp.tickers), dtype=bool)
    for ts in dates:
        pos = int(np.searchsorted(mp.date_ns, ts.value))
        big, big_caps = batch.select_universe(mp, pos, SIZES[-1], N, "daily", members)
        for ks in SIZES:
            cols, caps = batch.select_universe(mp, pos, ks, N, "daily", members)
            assert np.array_equal(cols, big[:ks]) and np.array_equal(caps, big_caps[:ks])
    batch.clear_panel_cache()


def test_calculate_weights_for_specs_still_refuses_mixed_sizes():
    from incorporating_different_sources_amd import portfolio_calculations as pc
    specs = [_spec("conjugate_hf_vix_vw", 8), _spec("conjugate_hf_vix_vw", 12)]
    for share in (False, True):
        with pytest.raises(ValueError) as e:
            pc.calculate_weights_for_specs([], specs, {}, share_grams=share)
        assert str(e.value) == "calculate_weights_for_specs: conjugate specs of equal size, window and frequencies expected"
    # the size axis has its own entry point, which refuses what it cannot share
    with pytest.raises(ValueError):
        pc.calculate_weights_for_sizes([], [_spec("conjugate_hf_vix_vw", 8), _spec("jeffreys", 12)], {})
    with pytest.raises(ValueError):
        pc.calculate_weights_for_sizes([], [_spec(k=8), dict(_spec(k=12), rolling_window=N + 1)], {})
    assert pc.calculate_weights_for_sizes([], [], {}) == []


def test_sizes_fall_back_spec_by_spec_when_the_largest_pack_raises(monkeypatch):
    """A date with fewer eligible stocks than the largest size: nothing is swept, every spec takes its own path (where the
    reference's exception surfaces for the sizes it applies to, and the smaller sizes are still served)."""
    from incorporating_different_sources_amd import portfolio_calculations as pc
    md, dates = _market(n_tickers=12)
    caps = md["stock_market_caps_df"].copy()
    caps.loc[dates[3], caps.columns[:2]] = np.nan                      # 10 stocks with a cap at that date
    md = dict(md, stock_market_caps_df=caps)
    specs = [_spec(k=4), _spec(k=8), _spec(k=12)]
    seen = []
    monkeypatch.setattr(pc, "_weights_for_dates", lambda d, sp, m: (seen.append(sp["size"]), (np.zeros((len(d), sp["size"])), [], None, None))[1])
    monkeypatch.setattr(pc, "_fill_spec_cache", lambda sps, d, m, w, n, same, lab, cols, cp: [(w, lab, cols, cp)])
    monkeypatch.setattr(_native, "Batch", lambda *a, **kw: pytest.fail("a device batch was created"))
    batch.clear_panel_cache()
    out = pc.calculate_weights_for_sizes(dates, specs, md)
    batch.clear_panel_cache()
    assert seen == [4, 8, 12] and [r[0].shape[1] for r in out] == [4, 8, 12]
