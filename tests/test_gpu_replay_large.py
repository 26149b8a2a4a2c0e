"""The device backtest replay above 8 slots per lane (-m gpu): `replay_kernel<16>` and `replay_kernel<32>` (513 <= k <= 2047),
whose rebalancing inputs are loaded after the day's reductions by a second copy of the load code, whose sum-check exit fills
the rest of the outputs with lane strides, and which the host's grouping launches as a fifth and a sixth class.

The yardstick is the long-double truth of tests/_replay_reference.py at the tolerance of tests/test_gpu_replay.py, RTOL = 1e-10
and ATOL = 1e-12; tests/_replay_cases.py derives it as a worst-case bound for the table's weights (gross exposure 2).
tests/test_host_replay_reference.py holds the host replay to a quarter of it on the same cases, without a GPU; the host is
compared here too, so that a failure names the side that moved.  Each test prints the worst ratio to the tolerance it saw.

1. every case of the table (classes' edges, degenerate shapes, input corners, 1,500 days) against the truth;
2. all six classes in one call: outputs land at the portfolio's own index, independent of the launch it shares;
3. the sum check at k = 513 and k = 2047 with two non-zero weights, where host and device round identically;
4. a sweep's download [W x P x L x S x k] at k = 700 replayed where it lies."""
import numpy as np
import pandas as pd
import pytest

import _replay_cases as rc
from _replay_cases import ATOL, METRIC_COLS, RTOL, _flat_call, _same_bytes, _universes
from _replay_reference import replay_reference_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    from incorporating_different_sources_amd import portfolio_calculations
    return portfolio_calculations


@pytest.fixture(scope="module")
def dev():
    from incorporating_different_sources_amd import _native
    return _native.default_device()


def _through_device_replay(case, pc, dev):
    """The case through `Device.replay` in its layout; per portfolio (returns[1:], turnover[1:], metrics)."""
    D, K, R, k = len(case.days), len(case.tickers), len(case.reb), case.k
    S = case.md["stock_simple_returns_df"].reindex(index=pd.DatetimeIndex(case.days), columns=case.tickers).to_numpy()
    if case.layout == "wide":
        S = np.concatenate([S, np.full((D, 3), 1e300)], axis=1)            # ld = K + 3: a read of the extra columns shows
    rows = 1 if case.layout == "one_row" else R
    stride = 0 if case.layout == "one_row" else k
    w_at, u_at, w_parts, c_parts, m_parts, w_off, u_off = {}, {}, [], [], [], [], []
    for w, cols, caps, _ in case.items:
        if id(w) not in w_at:
            w_at[id(w)] = rows * k * len(w_parts)
            w_parts.append(w[:rows].reshape(-1))
        if id(cols) not in u_at:
            u_at[id(cols)] = rows * k * len(c_parts)
            c_parts.append(cols[:rows].reshape(-1))
            m_parts.append(caps[:rows].reshape(-1))
        w_off.append(w_at[id(w)])
        u_off.append(u_at[id(cols)])
    P = len(case.items)
    day_of = {ts: d for d, ts in enumerate(case.days)}
    specs = [sp for _, _, _, sp in case.items]
    returns, turnover, metrics, status, bad_day = dev.replay(
        S=S, rf_daily=(pc._rf_asof(case.md["risk_free_rate_df"], case.days) + 1) ** (1 / 252) - 1,
        reb_day=np.array([day_of[ts] for ts in case.reb], dtype=np.int32), K=K, k=np.full(P, k, dtype=np.int32),
        scaling=np.array([sp["risk_aversion"] if sp["risk_aversion"] is not None else 1 for sp in specs], dtype=np.float64),
        cost=np.array([sp["turnover_cost"] for sp in specs], dtype=np.float64),
        w_off=np.array(w_off, dtype=np.int64), w_stride=np.full(P, stride, dtype=np.int64),
        u_off=np.array(u_off, dtype=np.int64), u_stride=np.full(P, stride, dtype=np.int64),
        weights=np.concatenate(w_parts), cols=np.concatenate(c_parts), caps=np.concatenate(m_parts))
    assert (status == 0).all() and (bad_day == -1).all()
    assert returns.shape == (P, D) and turnover.shape == (P, R) and metrics.shape == (P, R, 5)
    assert np.isnan(returns[:, 0]).all() and np.isnan(turnover[:, 0]).all()
    return [(returns[p, 1:], turnover[p, 1:], metrics[p]) for p in range(P)]


@pytest.mark.filterwarnings("ignore:Mean of empty slice")                 # a date whose caps are all NaN: the host's nanmean
@pytest.mark.parametrize("name", rc.LARGE)
def test_device_replay_against_the_truth(pc, dev, name):
    case, host, truth = rc.large_case(name), rc.large_host(name), rc.large_truth(name)
    if case.layout == "frames":
        frames = pc.replay_backtests_device(case.days, case.reb, case.items, case.md, tickers=case.tickers)
        assert len(frames) == len(host)
        for g, h in zip(frames, host):                                    # the host's indices, names, dtypes and columns
            for key in rc.SERIES:
                assert g[key].index.equals(h[key].index) and g[key].name == h[key].name and g[key].dtype == h[key].dtype
            gm, hm = g["portfolio_weights_metrics_df"], h["portfolio_weights_metrics_df"]
            assert gm.index.equals(hm.index) and list(gm.columns) == list(hm.columns) == METRIC_COLS
            assert gm.dtypes.equals(hm.dtypes)
        got = [rc.frames_to_arrays(g) for g in frames]
    else:
        got = _through_device_replay(case, pc, dev)
    worst = [0.0, 0.0, 0.0]
    for g, h, t, item in zip(got, host, truth, case.items):
        what = f"{name} {item[3]['display_name']}"
        h = rc.frames_to_arrays(h)
        ratios = rc.ratio(g, t, what + " device vs truth"), rc.ratio(h, t, what + " host vs truth"), rc.ratio(g, h, what)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
        assert rc.selections_equal(g[2], t[2]), f"{what}: max_long / max_short"
        assert ratios[0] <= 1, (f"{what}: device vs truth at {ratios[0]:.3g} of the tolerance (host vs truth {ratios[1]:.3g}, "
                                f"device vs host {ratios[2]:.3g})")
        for a, b, part in zip(g, h, ("returns", "turnover", "metrics")):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=f"{what} {part}: device vs host")
    print(f"{name}: worst ratio to the tolerance: device vs truth {worst[0]:.3e}, host vs truth {worst[1]:.3e}, "
          f"device vs host {worst[2]:.3e}")


SIX_CLASSES = ((1, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2047))


def _six_class_sizes():
    """41 sizes, 7 + 7 + 7 + 7 + 7 + 6 over the six classes (no count is a multiple of 4: every launch ends with a ragged
    workgroup), both edges of every class, dealt out so that the classes alternate: the sort by class moves every one."""
    stacks = [[pair[i % 2] for i in range(6 if pair[1] == 2047 else 7)] for pair in SIX_CLASSES]
    ks = []
    while any(stacks):
        for c in (5, 0, 4, 1, 3, 2):
            if stacks[c]:
                ks.append(stacks[c].pop())
    return ks


def test_six_classes_in_one_call(dev):
    rng = np.random.default_rng(66)
    ks = _six_class_sizes()
    spl = [next(s for s in (1, 2, 4, 8, 16, 32) if s * 64 >= k) for k in ks]
    assert len(ks) == 41 and set(ks) == {k for pair in SIX_CLASSES for k in pair}
    assert all(spl.count(s) % 4 != 0 for s in (1, 2, 4, 8, 16, 32))
    order = sorted(range(41), key=lambda p: spl[p])                       # (sorted is stable, like the host's sort)
    assert sum(p == q for p, q in enumerate(order)) <= 1, "the sort by class leaves portfolios where they are"
    kw = _flat_call(rng, D=40, K=4101, reb_day=[0, 1, 2, 7, 8, 20, 39], ks=ks)
    R = len(kw["reb_day"])
    blocks = []
    for p, k in enumerate(ks):                                            # gross exposure 2, as in the table
        at = int(kw["w_off"][p])
        kw["weights"][at:at + R * k] = rc.gross_two(kw["weights"][at:at + R * k].reshape(R, k)).reshape(-1)
        blocks.append(kw["weights"][at:at + R * k].reshape(R, k))
    assert len(set(kw["cost"])) > 1 and len(set(kw["scaling"])) > 1 and len(set(kw["u_off"])) >= 12
    first = dev.replay(**kw)
    returns, turnover, metrics, status, bad_day = first
    assert (status == 0).all() and (bad_day == -1).all()
    assert np.isnan(returns[:, 0]).all() and np.isnan(turnover[:, 0]).all()
    assert _same_bytes(first, dev.replay(**kw))
    worst = 0.0
    for p, k in enumerate(ks):
        alone = dict(kw)
        for name in ("k", "scaling", "cost", "w_off", "w_stride", "u_off", "u_stride"):
            alone[name] = kw[name][p:p + 1]
        assert _same_bytes([x[p:p + 1] for x in first], dev.replay(**alone)), f"portfolio {p} (k={k})"
        at = int(kw["u_off"][p])
        truth = replay_reference_arrays(kw["S"], kw["rf_daily"], kw["reb_day"], blocks[p],
                                        kw["cols"][at:at + R * k].reshape(R, k), kw["caps"][at:at + R * k].reshape(R, k),
                                        kw["scaling"][p], kw["cost"][p])
        got = (returns[p, 1:], turnover[p, 1:], metrics[p])
        r = rc.ratio(got, truth, f"portfolio {p} (k={k})")
        assert rc.selections_equal(got[2], truth[2]), f"portfolio {p} (k={k}): max_long / max_short"
        assert r <= 1, f"portfolio {p} (k={k}): device vs truth at {r:.3g} of the tolerance"
        worst = max(worst, r)
    print(f"six classes, 41 portfolios: device vs truth, worst ratio to the tolerance {worst:.3e}")


@pytest.mark.parametrize("reb_day", [(0, 2, 5), (0, 2, 3, 5)], ids=["wiped-out-between-dates", "wiped-out-on-a-date"])
def test_sum_check_above_eight_slots_per_lane(pc, dev, reb_day):
    """Case F of tests/test_gpu_replay.py at k = 513 and k = 2047, raising and passing candidates of both in one call (the
    waves that stop share workgroups with waves that go on).  In the second schedule the wipe-out day is a rebalancing day:
    the kernel stops before it rebalances, so that date's turnover and metrics are NaN."""
    found = {k: rc.wipe_out_candidates(k, reb_day) for k in (513, 2047)}
    per_k = []                                                            # (k, weights, the host's day or None)
    for k, (_, _, _, _, raised, passed) in found.items():
        assert len(raised) >= 5, f"k={k}: no candidate trips the host's check"
        assert len(passed) >= 5 and all(day == 3 for _, day in raised)
        per_k.append([(k, w, day) for pair in zip(raised, passed) for w, day in pair])      # raising, passing, raising, ...
    chosen = [c for pair in zip(*per_k) for c in pair]                    # k = 513, 2047, 513, ...
    (days, tickers, md, reb), _, _, spec, _, _ = found[513]
    S = md["stock_simple_returns_df"].to_numpy()
    rf = (pc._rf_asof(md["risk_free_rate_df"], days) + 1) ** (1 / 252) - 1
    R, P = len(reb_day), len(chosen)
    tables = {k: found[k][1] for k in found}
    u_at = {513: 0, 2047: R * 513}
    ks = np.array([k for k, _, _ in chosen], dtype=np.int32)
    w_len = np.array([R * k for k in ks], dtype=np.int64)
    returns, turnover, metrics, status, bad_day = dev.replay(
        S=S, rf_daily=rf, reb_day=np.array(reb_day, dtype=np.int32), K=rc.WIPE_OUT_TICKERS, k=ks, scaling=np.ones(P),
        cost=np.full(P, 15.0), w_off=np.concatenate([[0], np.cumsum(w_len)[:-1]]).astype(np.int64), w_stride=ks.astype(np.int64),
        u_off=np.array([u_at[k] for k in ks], dtype=np.int64), u_stride=ks.astype(np.int64),
        weights=np.concatenate([w.reshape(-1) for _, w, _ in chosen]),
        cols=np.concatenate([tables[513].reshape(-1), tables[2047].reshape(-1)]), caps=np.ones(R * (513 + 2047)))
    assert 0 < int((status != 0).sum()) < P
    for p, (k, w, day) in enumerate(chosen):
        what = f"portfolio {p} (k={k})"
        if day is None:
            assert status[p] == 0 and bad_day[p] == -1, what
            n_days, j0 = len(days), R
        else:
            assert status[p] == 1 and bad_day[p] == day, what
            j0 = next(j for j in range(R) if reb_day[j] >= day)           # the first rebalancing date that is not reached
            assert np.isfinite(returns[p, 1:day]).all() and np.isnan(returns[p, day:]).all(), what
            assert np.isfinite(turnover[p, 1:j0]).all() and np.isnan(turnover[p, j0:]).all(), what
            assert np.isfinite(metrics[p, :j0, 4]).all() and np.isnan(metrics[p, j0:]).all(), what
            n_days = day
        with np.errstate(all="ignore"):                                   # what the host has of it (all of it, if it passes)
            want = pc._replay_backtest(days[:n_days], reb[:j0], w, tables[k], np.ones((R, k)), tickers, spec, md)
        for a, b in zip((returns[p, 1:n_days], turnover[p, 1:j0], metrics[p, :j0]), rc.frames_to_arrays(want)):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=what)
    print(f"sum check {reb_day}: {int((status != 0).sum())} of {P} portfolios stopped on day 3")
    k, w, _ = next(c for c in chosen if c[2] is not None)
    with pytest.raises(ValueError, match="Weights do not sum to 1."):
        pc.replay_backtests_device(days, reb, [(w, tables[k], np.ones((R, k)), spec)], md, tickers=tickers)


def test_sweep_download_at_large_k_is_replayed_where_it_lies(dev):
    """Case D of tests/test_gpu_replay.py with k = 700 and sizes [150, 700]: 4 and 16 slots per lane side by side.  In place
    and packed densely must agree byte for byte; two layouts that agree could still both be wrong, so every entry is also
    held against the truth (rows of gross exposure 2, as in the table)."""
    rng = np.random.default_rng(45)
    W, P, L, sizes, k, K, D = 6, 2, 3, [150, 700], 700, 1600, 30
    n_s = len(sizes)
    grid = np.zeros((W, P, L, n_s, k))
    for s, ks in enumerate(sizes):
        grid[..., s, :ks] = rc.gross_two(rng.normal(0.01, 0.3, (W, P, L, ks)))
    cols = _universes(rng, W, k, K)
    caps = rng.lognormal(3, 1, (W, k))
    S = rng.normal(0.0005, 0.02, (D, K))
    entries = [(p, l, s) for p in range(P) for l in range(L) for s in range(n_s)]
    n = len(entries)
    shared = dict(S=S, rf_daily=np.full(D, 0.0001), reb_day=np.array([0, 4, 9, 10, 21, 29], dtype=np.int32), K=K,
                  k=np.array([sizes[s] for _, _, s in entries], dtype=np.int32), scaling=np.full(n, 5.0),
                  cost=np.full(n, 15.0), u_off=np.zeros(n, dtype=np.int64), u_stride=np.full(n, k, dtype=np.int64),
                  cols=cols, caps=caps)
    in_place = dev.replay(weights=grid, w_off=np.array([((p * L + l) * n_s + s) * k for p, l, s in entries], dtype=np.int64),
                          w_stride=np.full(n, P * L * n_s * k, dtype=np.int64), **shared)
    dense = np.concatenate([grid[:, p, l, s, :sizes[s]].reshape(-1) for p, l, s in entries])
    lens = np.array([W * sizes[s] for _, _, s in entries], dtype=np.int64)
    packed = dev.replay(weights=dense, w_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64),
                        w_stride=shared["k"].astype(np.int64), **shared)
    assert (in_place[3] == 0).all() and np.isfinite(in_place[0][:, 1:]).all()
    assert _same_bytes(in_place, packed)
    worst = 0.0
    for e, (p, l, s) in enumerate(entries):                               # and it is the right replay: against the truth
        truth = replay_reference_arrays(S, shared["rf_daily"], shared["reb_day"], grid[:, p, l, s, :sizes[s]],
                                        cols[:, :sizes[s]], caps[:, :sizes[s]], 5.0, 15.0)
        got = (in_place[0][e, 1:], in_place[1][e, 1:], in_place[2][e])
        r = rc.ratio(got, truth, f"entry {(p, l, s)}")
        assert rc.selections_equal(got[2], truth[2]) and r <= 1, f"entry {(p, l, s)}: device vs truth at {r:.3g} of the tolerance"
        worst = max(worst, r)
    print(f"sweep layout, k = 150 and 700: device vs truth, worst ratio to the tolerance {worst:.3e}")
