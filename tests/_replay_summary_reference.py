"""The truth and the cases of the replay summary's tests (tests/test_host_replay_summary.py, CPU; tests/test_gpu_replay_summary.py,
GPU).  No tests in here.

`summary_truth` takes what a replay stored - returns [P x D], turnover [P x R] - and forms the series exactly as
include/tangency_posterior.h (tp_replay_summary) defines them, in double: the net return, the excess return.  Everything after
that is restated plainly in numpy.longdouble: the compounded wealth as a sequential product, the adjusted day's value
(rounded to double, since the series are doubles), and every statistic.

Tolerance: the replay tests' RTOL = 1e-10, ATOL = 1e-12, as a bound.  A sum of n <= 4,095 terms in any order errs by at most
(n - 1) 2^-53 sum|terms|, a product of n factors by about n 2^-53 relative; at n = 700 that is 8e-14, a thousandth of RTOL.  For
the sums whose terms cancel - the means (MEAN, MEAN_PRE, MEAN_E), M3_E and SUM_NONZERO - the relative part is taken against
sum|terms| / n, which `summary_truth` also returns (`scale`); for every other field against |truth|.  The wealth-based fields
(COMP, MAX_DD) are differences from 1 of quantities with that relative error: ATOL covers them.  The host yardstick
(`summary_records_host`) gets a quarter of the tolerance, the device the whole.

A condition on the cases (`Truth.margin_ok`, asserted for every (case, portfolio, cost); a case that violates it is a failure
of the builder): wherever a comparison of the wealth decides something, the wealth is farther than 1e-9 from the threshold, so
that no summation order can decide otherwise - W_d from 0 on every day up to and including the adjusted day (the series before
its adjustment: "W - 1 < -1" is never evaluated again after it, ref:70, and W is then exactly 0 when day 1 was adjusted), for
a and for b; W_d of a from 0.01 on every day; and no |a_d| within 1e-12 of 1e-7."""
import functools

import numpy as np

from _replay_reference import LD, replay_reference_arrays

RTOL, ATOL = 1e-10, 1e-12
NSTATS = 32
(N_OBS, ADJ_DAY, INSOLVENT_DAY, COMP, MEAN, STD, MAX_DD, BEST, WORST, SUM_WIN, N_WIN, SUM_LOSS, N_LOSS, N_PRE, MEAN_PRE, STD_PRE,
 WORST_PRE, SUM_NONZERO, N_NONZERO, ADJ_DAY_E, MEAN_E, STD_E, M2_E, M3_E, M4_E, DOWNSIDE_E, TURNOVER_SUM, TURNOVER_N) = range(28)
EXACT = (N_OBS, ADJ_DAY, INSOLVENT_DAY, N_WIN, N_LOSS, N_PRE, N_NONZERO, ADJ_DAY_E, TURNOVER_N)     # day indices and counts
KEPT = (N_OBS, ADJ_DAY, INSOLVENT_DAY, ADJ_DAY_E)
OK, NO_REPLAY, NONFINITE = 0, 1, 2
_NAN = LD("nan")


def net_and_excess(ret, turn, reb_day, cost, rf_excess):
    """x [D-1] and e [D-1] of one portfolio and one cost, in double, one rounding per operation."""
    with np.errstate(all="ignore"):
        x = np.array(ret[1:], dtype=np.float64)
        charged = np.asarray(reb_day[1:], dtype=np.int64)
        x[charged - 1] = ret[charged] - (np.float64(cost) / np.float64(10000)) * turn[1:]
        return x, x - np.asarray(rf_excess, dtype=np.float64)[1:]


def _wealth(v):
    w = np.empty(v.size, dtype=LD)
    acc = LD(1)
    for i, f in enumerate(1 + v.astype(LD)):
        acc = acc * f
        w[i] = acc
    return w


def _first(mask):
    hit = np.flatnonzero(mask)
    return int(hit[0]) if hit.size else -1


def _adjusted(v):
    """(the adjusted series as doubles, index of the changed entry or -1, min |W| over the days where W < 0 was asked)."""
    with np.errstate(all="ignore"):
        w = _wealth(v)
        i = _first(w - 1 < -1)
        asked = w if i < 0 else w[:i + 1]
        margin = float(np.min(np.abs(asked))) if not np.isnan(asked.astype(np.float64)).any() else np.inf
        if i < 0:
            return v, -1, margin
        out = v.copy()
        out[i] = -1.0 if i == 0 else np.float64(LD(np.float64(0.000001)) / (w[i - 1] - 1) - 1)
        out[i + 1:] = 0.0
        return out, i, margin


def _std(v, mean):
    return np.sqrt(((v - mean) ** 2).sum(dtype=LD) / (v.size - 1)) if v.size >= 2 else _NAN


class Truth:
    """stats, scale [P x C x 32] (long double), status [P x C], margin_ok [P x C]."""

    def __init__(self, P, C):
        self.stats = np.zeros((P, C, NSTATS), dtype=LD)
        self.scale = np.zeros((P, C, NSTATS), dtype=LD)
        self.status = np.zeros((P, C), dtype=np.int32)
        self.margin_ok = np.ones((P, C), dtype=bool)


def summary_truth(ret, turn, reb_day, cost_bp, rf_excess, replay_status=None):
    ret, turn = np.asarray(ret, dtype=np.float64), np.asarray(turn, dtype=np.float64)
    reb_day = np.asarray(reb_day, dtype=np.int64)
    P, D = ret.shape
    n = D - 1
    t = Truth(P, len(cost_bp))
    with np.errstate(all="ignore"):
        for p in range(P):
            if replay_status is not None and replay_status[p] != 0:
                t.stats[p, :, :28] = _NAN
                t.status[p] = NO_REPLAY
                continue
            for c, cost in enumerate(cost_bp):
                x, e = net_and_excess(ret[p], turn[p], reb_day, cost, rf_excess)
                a, adj_a, margin_a = _adjusted(x)
                b, adj_b, margin_b = _adjusted(e)
                w = _wealth(a)
                ins = _first(w - 1 < -0.99)
                s = t.stats[p, c]
                s[N_OBS], s[ADJ_DAY], s[INSOLVENT_DAY], s[ADJ_DAY_E] = n, adj_a + 1 if adj_a >= 0 else -1, \
                    ins + 1 if ins >= 0 else -1, adj_b + 1 if adj_b >= 0 else -1
                if not (np.isfinite(a).all() and np.isfinite(b).all()):
                    s[[i for i in range(28) if i not in KEPT]] = _NAN
                    t.status[p, c] = NONFINITE
                    continue
                t.margin_ok[p, c] = (margin_a > 1e-9 and margin_b > 1e-9 and float(np.min(np.abs(w - LD(0.01)))) > 1e-9
                                     and float(np.min(np.abs(np.abs(a) - 1e-7))) > 1e-12)
                al, bl = a.astype(LD), b.astype(LD)
                pre = al if ins < 0 else al[:ins]
                s[COMP] = w[-1] - 1
                s[MEAN] = al.sum(dtype=LD) / n
                s[STD] = _std(al, s[MEAN])
                s[MAX_DD] = np.min(w / np.maximum.accumulate(w) - 1)
                s[BEST], s[WORST] = al.max(), al.min()
                s[SUM_WIN], s[N_WIN] = al[al > 0].sum(dtype=LD), (al > 0).sum()
                s[SUM_LOSS], s[N_LOSS] = al[al < 0].sum(dtype=LD), (al < 0).sum()
                s[N_PRE] = pre.size
                s[MEAN_PRE] = pre.sum(dtype=LD) / pre.size if pre.size else _NAN
                s[STD_PRE] = _std(pre, s[MEAN_PRE])
                s[WORST_PRE] = pre.min() if pre.size else _NAN
                moved = np.abs(al) > 1e-7
                s[SUM_NONZERO], s[N_NONZERO] = al[moved].sum(dtype=LD), moved.sum()
                s[MEAN_E] = bl.sum(dtype=LD) / n
                centred = bl - s[MEAN_E]
                s[STD_E] = _std(bl, s[MEAN_E])
                s[M2_E], s[M3_E], s[M4_E] = ((centred ** q).sum(dtype=LD) / n for q in (2, 3, 4))
                s[DOWNSIDE_E] = (bl[bl < 0] ** 2).sum(dtype=LD) / n
                traded = turn[p, 1:].astype(LD)
                if ins >= 0:
                    traded = traded[reb_day[1:] <= ins + 1]
                s[TURNOVER_SUM], s[TURNOVER_N] = traded.sum(dtype=LD), traded.size
                sc = t.scale[p, c]
                sc[:] = np.abs(s)
                sc[MEAN] = np.abs(al).sum(dtype=LD) / n
                sc[MEAN_PRE] = np.abs(pre).sum(dtype=LD) / pre.size if pre.size else 0
                sc[MEAN_E] = np.abs(bl).sum(dtype=LD) / n
                sc[M3_E] = (np.abs(centred) ** 3).sum(dtype=LD) / n
                sc[SUM_NONZERO] = np.abs(al[moved]).sum(dtype=LD) / n
    return t


def ratio(stats, status, truth, what=""):
    """max |got - truth| / (ATOL + RTOL scale) over the records.  Statuses, NaN positions, day indices and counts must be equal
    (asserted here); no entry may be infinite."""
    got = np.asarray(stats, dtype=LD)
    assert got.shape == truth.stats.shape, f"{what}: shape {got.shape}, expected {truth.stats.shape}"
    assert np.array_equal(np.asarray(status), truth.status), f"{what}: statuses {np.asarray(status).tolist()}, expected {truth.status.tolist()}"
    odd = np.isnan(got) != np.isnan(truth.stats)
    assert not odd.any(), f"{what}: NaN at other fields than in the truth: {sorted(set(np.argwhere(odd)[:, 2].tolist()))}"
    assert np.array_equal(got[..., list(EXACT)], truth.stats[..., list(EXACT)], equal_nan=True), f"{what}: a day index or a count differs"
    assert (got[..., 28:] == 0).all(), f"{what}: a reserved field is not 0.0"
    ok = ~np.isnan(truth.stats)
    assert np.isfinite(got[ok].astype(np.float64)).all(), f"{what}: an infinite entry"
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - truth.stats[ok]) / (ATOL + RTOL * truth.scale[ok])).max())


# ---------------------------------------------------------------------------------------------------------------------------
# cases: replays of fully invested long-only portfolios over one universe, so that on a day when every asset returns the same
# value c (a "shock") every portfolio returns c to rounding, whatever it holds
COSTS = {1: [0.0], 3: [0.0, 15.0, 35.0], 4: [0.0, 5.0, 15.0, 35.0], 5: [0.0, 5.0, 10.0, 15.0, 35.0],
         9: [0.0, 1.0, 2.0, 5.0, 10.0, 15.0, 20.0, 25.0, 35.0]}


def schedule(D, kind):
    return np.array({"none": [0], "monthly": list(range(0, D, 21)), "daily": list(range(D))}[kind], dtype=np.int32)


class Case:
    """`call`: the arguments of `Device.replay` (cost 0 for every portfolio); `cost_bp`, `rf_excess`: those of the summary;
    `expect`: {field: value} every (portfolio, cost) of the truth must show, or {field: [values per cost]}."""

    def __init__(self, name, call, cost_bp, rf_excess, expect=None, expect_status=None):
        self.name, self.call, self.rf_excess = name, call, rf_excess
        self.cost_bp = np.array(cost_bp, dtype=np.float64)
        self.expect, self.expect_status = expect or {}, expect_status

    def __repr__(self):
        return self.name


def _call(D, reb_day, P, k, seed, shocks=None, flat_days=()):
    rng = np.random.default_rng(seed)
    R = len(reb_day)
    S = rng.normal(0.0005, 0.02, (D, k))
    rf_daily = 0.0001 * rng.random(D)
    for d, c in (shocks or {}).items():
        S[d] = c
    for d in flat_days:
        S[d], rf_daily[d] = 0.0, 0.0
    w = np.abs(rng.normal(0.0, 1.0, (P, R, k))) + 0.05
    w /= w.sum(axis=2, keepdims=True)
    ks = np.full(P, k, dtype=np.int32)
    return dict(S=S, rf_daily=rf_daily, reb_day=np.asarray(reb_day, dtype=np.int32), K=k, k=ks, scaling=np.ones(P), cost=np.zeros(P),
                w_off=np.arange(P, dtype=np.int64) * R * k, w_stride=ks.astype(np.int64), u_off=np.zeros(P, dtype=np.int64),
                u_stride=ks.astype(np.int64), weights=w.reshape(-1), cols=np.tile(np.arange(k, dtype=np.int32), R),
                caps=np.ones(R * k))


def _rf(D, seed, **at):
    rf = 0.0001 + 0.00002 * np.random.default_rng(seed + 1).random(D)
    for d, v in at.items():
        rf[int(d[1:])] = v
    return rf


def _generic(name, D, kind, P, C, k=4, seed=0, call=None, rf=None, **expectations):
    return Case(name, _call(D, schedule(D, kind), P, k, 100 + seed + D, **(call or {})), COSTS[C], _rf(D, seed + D, **(rf or {})),
                **expectations)


def _two_highest_costs(name):
    """Day 42, a rebalancing day, returns -1 + 10 bp x its turnover: 1 + x stays positive at 0 and 5 bp and is negative at 15
    and 35 bp.  With every asset returning the same the drifted weights, and so the turnover, do not depend on that return."""
    D, reb = 130, schedule(130, "monthly")
    probe = _call(D, reb, 1, 4, 4242, shocks={42: -0.5})
    turn = host_replay(probe)[1][0]
    c = -1 + 0.001 * float(turn[2])
    return Case(name, _call(D, reb, 1, 4, 4242, shocks={42: c}), COSTS[4], _rf(D, 4242),
                expect={ADJ_DAY: [-1, -1, 42, 42], INSOLVENT_DAY: 42})


def _nan_turnover(name):
    """Portfolio 2 holds +inf and -inf from rebalancing date 2 (day 42) on: its turnover there is NaN and so is the return the
    replay itself stores (0 x NaN at cost 0), for every cost."""
    case = _generic(name, 130, "monthly", 5, 3, seed=7)
    w = case.call["weights"].reshape(5, -1, 4)
    w[2, 2, 0], w[2, 2, 1] = np.inf, -np.inf
    case.expect_status = np.array([[OK] * 3, [OK] * 3, [NONFINITE] * 3, [OK] * 3, [OK] * 3], dtype=np.int32)
    return case


_BUILDERS = {
    # shapes: D = 2 (n = 1), 3, 64, 65, 66, 129, 130, 700; R = 1, monthly, daily; C = 1, 3, 5, 9; P = 1, 5, 37
    "D2-none-P1-C1": functools.partial(_generic, D=2, kind="none", P=1, C=1),
    "D2-daily-P5-C3": functools.partial(_generic, D=2, kind="daily", P=5, C=3),
    "D3-daily-P1-C5": functools.partial(_generic, D=3, kind="daily", P=1, C=5),
    "D64-monthly-P5-C9": functools.partial(_generic, D=64, kind="monthly", P=5, C=9),
    "D65-monthly-P37-C3": functools.partial(_generic, D=65, kind="monthly", P=37, C=3),
    "D66-daily-P5-C5": functools.partial(_generic, D=66, kind="daily", P=5, C=5),
    "D129-monthly-P1-C9": functools.partial(_generic, D=129, kind="monthly", P=1, C=9),
    "D130-daily-P5-C1": functools.partial(_generic, D=130, kind="daily", P=5, C=1),
    "D700-monthly-P37-C5": functools.partial(_generic, D=700, kind="monthly", P=37, C=5, expect={ADJ_DAY: -1, INSOLVENT_DAY: -1}),
    "D700-daily-P5-C9": functools.partial(_generic, D=700, kind="daily", P=5, C=9),
    "D700-none-P5-C3": functools.partial(_generic, D=700, kind="none", P=5, C=3),
    "k513-D66-monthly-P1-C3": functools.partial(_generic, D=66, kind="monthly", P=1, C=3, k=513),
    # the adjusted day: day 1, lane 63 of tile 0, lane 0 of tile 1 (day 65), lane 63 of tile 1, the last day
    "adjust-day1": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, call=dict(shocks={1: -2.5}),
                                     expect={ADJ_DAY: 1, INSOLVENT_DAY: 1, N_PRE: 0}),
    "adjust-day64": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, call=dict(shocks={64: -2.5}),
                                      expect={ADJ_DAY: 64, INSOLVENT_DAY: 64}),
    "adjust-day65": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, call=dict(shocks={65: -2.5}),
                                      expect={ADJ_DAY: 65, INSOLVENT_DAY: 65}),
    "adjust-day128": functools.partial(_generic, D=130, kind="daily", P=5, C=3, call=dict(shocks={128: -2.5}),
                                       expect={ADJ_DAY: 128, INSOLVENT_DAY: 128}),
    "adjust-last-day": functools.partial(_generic, D=130, kind="monthly", P=1, C=5, call=dict(shocks={129: -2.5}),
                                         expect={ADJ_DAY: 129, INSOLVENT_DAY: 129}),
    # insolvency before the adjusted day (on it: every case above; never: the shapes)
    "insolvent-before-adjust": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, call=dict(shocks={30: -0.995, 70: -2.5}),
                                                 expect={ADJ_DAY: 70, INSOLVENT_DAY: 30}),
    "insolvent-not-adjusted": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, call=dict(shocks={30: -0.995}),
                                                expect={ADJ_DAY: -1, INSOLVENT_DAY: 30}),
    "adjust-two-highest-costs": _two_highest_costs,
    # 1 + x = 0.001 stays positive, 1 + x - rf_excess = -0.001 does not
    "excess-adjusted-alone": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, call=dict(shocks={50: -0.999}),
                                               rf=dict(d50=0.002), expect={ADJ_DAY: -1, ADJ_DAY_E: 50, INSOLVENT_DAY: 50}),
    "adjust-on-rebalancing-day": functools.partial(_generic, D=130, kind="monthly", P=5, C=5, call=dict(shocks={63: -2.5}),
                                                   expect={ADJ_DAY: 63, INSOLVENT_DAY: 63}),
    # days 1 and 2 return exactly 0: prev_cum_return is 0 and the adjusted value infinite, as the reference wrote it
    "zero-prev-cum-return": functools.partial(_generic, D=66, kind="none", P=5, C=3, call=dict(shocks={3: -2.5}, flat_days=(1, 2)),
                                              expect={ADJ_DAY: 3, ADJ_DAY_E: 3}, expect_status=np.full((5, 3), NONFINITE, dtype=np.int32)),
    "rf-excess-nan": functools.partial(_generic, D=130, kind="monthly", P=5, C=3, rf=dict(d40=np.nan),
                                       expect_status=np.full((5, 3), NONFINITE, dtype=np.int32)),
    "turnover-nan": _nan_turnover,
}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name](name)


def host_replay(call):
    """(returns [P x D], turnover [P x R], status [P]) of a case's replay on the CPU: the long-double replay of
    tests/_replay_reference.py rounded to double (entry 0 of each row is NaN, as the device stores it)."""
    P, D, R = call["k"].size, call["S"].shape[0], call["reb_day"].size
    ret, turn = np.full((P, D), np.nan), np.full((P, R), np.nan)
    for p in range(P):
        k = int(call["k"][p])
        rows = lambda a, off, st: np.stack([a[off + j * st: off + j * st + k] for j in range(R)])   # noqa: E731
        r, t, _m = replay_reference_arrays(call["S"], call["rf_daily"], call["reb_day"],
                                           rows(call["weights"], int(call["w_off"][p]), int(call["w_stride"][p])),
                                           rows(call["cols"], int(call["u_off"][p]), int(call["u_stride"][p])),
                                           rows(call["caps"], int(call["u_off"][p]), int(call["u_stride"][p])), cost=call["cost"][p])
        ret[p, 1:], turn[p, 1:] = r.astype(np.float64), t.astype(np.float64)
    return ret, turn, np.zeros(P, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(returns, turnover, truth) of a case from the CPU replay.  Computed once; do not modify."""
    c = case(name)
    ret, turn, _st = host_replay(c.call)
    return ret, turn, summary_truth(ret, turn, c.call["reb_day"], c.cost_bp, c.rf_excess)


def check_case(c, truth):
    """The margin condition, and that the case shows what its name says."""
    assert truth.margin_ok.all(), f"{c.name}: the margin condition fails at (portfolio, cost) {np.argwhere(~truth.margin_ok).tolist()}"
    if c.expect_status is not None:
        assert np.array_equal(truth.status, c.expect_status), f"{c.name}: statuses {truth.status.tolist()}"
    for field, want in c.expect.items():
        got = truth.stats[..., field].astype(np.float64)
        assert np.array_equal(got, np.broadcast_to(np.asarray(want, dtype=np.float64), got.shape)), \
            f"{c.name}: field {field} is {got.tolist()}, the case expects {want}"
