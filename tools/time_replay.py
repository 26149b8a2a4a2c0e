#!/usr/bin/env python3
"""The device backtest replay against the host loop it stands in for, both sides in one process on one box.

    python tools/time_replay.py [--portfolios 256] [--k 100] [--days 2500] [--freqs monthly,daily] [--reps 3]
                                [--host-portfolios 8] [--out FILE]

A synthetic grid: `--portfolios` portfolios of `--k` assets over `--days` business days, random long / short weights at
every rebalancing date, universes that change a few tickers per date, eight portfolios per universe table.

  "host"    one `_replay_backtest` per portfolio (the Python loop over trading days); timed on `--host-portfolios` of them
            and scaled to the grid (the loop is the same work for every portfolio; the scale factor is printed);
  "device"  one `replay_backtests_device` call for the whole grid, timed two ways: kernel ms from the handle's HIP events
            (tp_last_timing), and wall ms of the call - packing, merge maps, upload, launch, download, result frames.

Medians of `--reps` repetitions after one warm-up of each side, the two sides alternated inside each repetition.  The
results are compared before any time is reported.  Per-day cost of the kernel: kernel ms / days - the loop is sequential in
days, so with few portfolios per launch this is the latency of one day's dependent chain (two reduction rounds), not a
throughput.  One process, one device; run it under a time limit.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def build_grid(P, k, D, freq, seed):
    import numpy as np
    import pandas as pd
    from incorporating_different_sources_amd import portfolio_calculations as pc
    rng = np.random.default_rng(seed)
    K = 5 * k
    days = [pd.Timestamp(d) for d in pd.bdate_range("2010-01-04", periods=D)]
    tickers = [f"T{i:04d}" for i in range(K)]
    md = {"stock_simple_returns_df": pd.DataFrame(rng.normal(0.0004, 0.015, (D, K)), index=pd.DatetimeIndex(days), columns=tickers),
          "risk_free_rate_df": pd.DataFrame({"rf": np.full(D, 0.02)}, index=pd.DatetimeIndex(days))}
    reb = pc.rebalancing_schedule(days, freq)
    R = len(reb)
    tables = []
    for _ in range((P + 7) // 8):
        cols = np.empty((R, k), dtype=np.int32)
        cur = rng.permutation(K)[:k]
        for j in range(R):
            free = np.setdiff1d(np.arange(K), cur)
            at = rng.permutation(k)[:3]
            cur = cur.copy()
            cur[at] = rng.permutation(free)[:3]
            cols[j] = cur
        tables.append((cols, rng.lognormal(3, 1, (R, k))))
    items = []
    for p in range(P):
        cols, caps = tables[p // 8]
        w = rng.normal(0.01, 0.05, (R, k))
        spec = {"weighting_strategy": "grid", "size": k, "risk_aversion": [1, 2.5, 5][p % 3], "turnover_cost": 5 * (p % 8),
                "rebalancing_frequency": freq, "rolling_window": 250, "rolling_window_frequency": "daily",
                "mcm_scaling": 1, "display_name": f"p{p}"}
        items.append((w, cols, caps, spec))
    return days, reb, tickers, md, items


def measure(P, k, D, freq, reps, host_n, out):
    import numpy as np
    from incorporating_different_sources_amd import _native, portfolio_calculations as pc
    days, reb, tickers, md, items = build_grid(P, k, D, freq, seed=D + k)
    dev = _native.default_device()
    host_n = min(host_n, P)

    def host():
        t0 = time.perf_counter()
        res = [pc._replay_backtest(days, reb, w, c, m, tickers, sp, md) for w, c, m, sp in items[:host_n]]
        return res, (time.perf_counter() - t0) * 1e3

    def device():
        t0 = time.perf_counter()
        res = pc.replay_backtests_device(days, reb, items, md, tickers=tickers, device=dev)
        wall = (time.perf_counter() - t0) * 1e3
        return res, wall, dev.last_timing()["kernel_ms"]

    h_res, _ = host()                                                     # warm-up of both sides, and the comparison
    d_res, _, _ = device()
    worst = 0.0
    for h, d in zip(h_res, d_res):
        for key in h:
            a, b = np.asarray(h[key], dtype=float), np.asarray(d[key], dtype=float)
            if not np.allclose(a, b, rtol=1e-9, atol=1e-12, equal_nan=True):
                raise SystemExit(f"{freq}: the device replay disagrees with the host in {key}")
            both = np.isfinite(a) & np.isfinite(b)
            worst = max(worst, float(np.abs(a[both] - b[both]).max()) if both.any() else 0.0)
    host_ms, wall_ms, kernel_ms = [], [], []
    for _ in range(reps):
        host_ms.append(host()[1])
        _, wall, kern = device()
        wall_ms.append(wall)
        kernel_ms.append(kern)
    h, w, kn = statistics.median(host_ms), statistics.median(wall_ms), statistics.median(kernel_ms)
    scale = P / host_n
    lines = [f"{freq}: P={P} k={k} days={D} rebalancing dates={len(reb)}  max |host - device| = {worst:.2e}",
             f"  host    {h:10.1f} ms for {host_n} portfolios ({h / host_n / (D - 1) * 1e3:.1f} us per portfolio-day)"
             f"  -> x{scale:g} = {h * scale:10.1f} ms for the grid (scaled, not measured)",
             f"  device  {kn:10.3f} ms kernel ({kn / (D - 1) * 1e3:.2f} us per trading day of the launch), {w:10.1f} ms wall"
             f"  [kernel spread {min(kernel_ms):.3f}-{max(kernel_ms):.3f}, wall spread {min(wall_ms):.1f}-{max(wall_ms):.1f}]",
             f"  host / device kernel = {h * scale / kn:.0f}x   host / device wall = {h * scale / w:.1f}x"]
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--portfolios", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--days", type=int, default=2500)
    ap.add_argument("--freqs", default="monthly,daily")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-portfolios", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None
    for freq in args.freqs.split(","):
        measure(args.portfolios, args.k, args.days, freq, args.reps, args.host_portfolios, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()
