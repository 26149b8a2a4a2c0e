#!/usr/bin/env python3
"""The device-fed backtest replay (`Batch.replay`, tp_replay_run_batch) against the path it replaces, both in one process on
one box, on the same portfolios over the same grid sweep.

    python tools/time_replay_batch.py [--portfolios 256] [--k 100] [--days 2500] [--freqs monthly,daily] [--reps 5]
                                      [--patched 0.05] [--out FILE]

One conjugate batch of W = rebalancing dates windows at `--k` assets and ONE grid sweep of 16 priors x 16 lengths at size k
(256 entries per window; `--portfolios` portfolios read them round robin and differ in cost, scaling and risk aversion, eight
to a universe table).  The sweep is finished (`Device.synchronize`) before either side's clock starts; neither side changes
its results.

  "download"  the parent's path: tp_batch_download_grid_sweep -> pack (one contiguous [R x k] table per portfolio, scaled by
              1.0 / g as `calculate_weights_for_grid` does, concatenated as `replay_backtests_device` does) -> tp_replay_run ->
              tp_replay_download;
  "in place"  tp_replay_run_batch (offsets into the sweep's buffer, a scale per portfolio) -> tp_replay_download.

Per side: wall ms from the end of the sweep to the results on the host, and kernel ms of the replay from the handle's HIP
events (tp_last_timing).  Then the same with `--patched` of all (portfolio, date) pairs patched: rows substituted on the host on
the one side, patch rows on the other.  Medians of `--reps` repetitions after one warm-up of each side, the sides alternated
inside each repetition, min - max next to every median.  The results of the two sides are compared byte for byte before any
time is reported.  One process, one device; run it under a time limit.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N_PRIOR, N_LEN = 16, 16


def build(P, k, D, freq, seed):
    import numpy as np
    import pandas as pd
    from incorporating_different_sources_amd import _native, portfolio_calculations as pc, synthetic
    rng = np.random.default_rng(seed)
    days = [pd.Timestamp(d) for d in pd.bdate_range("2010-01-04", periods=D)]
    reb = pc.rebalancing_schedule(days, freq)
    day_of = {ts: d for d, ts in enumerate(days)}
    reb_day = np.array([day_of[ts] for ts in reb], dtype=np.int32)
    R = len(reb)
    N = 250
    inp = synthetic.make_kernel_inputs(k, N, R, seed=seed, hf_period=8)
    Nl = np.linspace(k + 30, N, N_LEN).astype(np.int32)
    rows = np.tile((Nl - 1).astype(np.int32), (R, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(R, N_PRIOR, N_LEN))
    w0 = rng.dirichlet(np.ones(k), size=(R, N_PRIOR))[:, :, None, :]
    dev = _native.default_device()
    b = dev.batch("conjugate", k, N, inp["n_r"], 1.0, R, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    _, status, _ = b.grid_sweep([k], Nl, rows, n0, np.ascontiguousarray(w0), want_aux=False, want_weights=False)
    if (status != 0).any():
        raise SystemExit("the sweep flagged an entry")
    dev.synchronize()
    K = 5 * k
    cols_parts, caps_parts = [], []
    for _ in range((P + 7) // 8):
        cols = np.empty((R, k), dtype=np.int32)
        cur = rng.permutation(K)[:k]
        for j in range(R):
            free = np.setdiff1d(np.arange(K), cur)
            at = rng.permutation(k)[:3]
            cur = cur.copy()
            cur[at] = rng.permutation(free)[:3]
            cols[j] = cur
        cols_parts.append(cols.reshape(-1))
        caps_parts.append(rng.lognormal(3, 1, R * k))
    entries = N_PRIOR * N_LEN
    entry = np.arange(P, dtype=np.int64) % entries
    gammas = np.array([[1.0, 2.5, 5.0][p % 3] for p in range(P)])
    call = dict(S=rng.normal(0.0004, 0.015, (D, K)), rf_daily=np.full(D, (1 + 0.02) ** (1 / 252) - 1), reb_day=reb_day, K=K,
                k=np.full(P, k, dtype=np.int32), scaling=gammas, cost=np.array([5.0 * (p % 8) for p in range(P)]),
                u_off=(np.arange(P, dtype=np.int64) // 8) * R * k, u_stride=np.full(P, k, dtype=np.int64),
                cols=np.concatenate(cols_parts), caps=np.concatenate(caps_parts))
    where = dict(w_off=entry * k, w_stride=np.full(P, entries * k, dtype=np.int64), s_off=entry,
                 s_stride=np.full(P, entries, dtype=np.int64))
    return dev, b, call, where, gammas, R


def measure(P, k, D, freq, reps, patched, out, record):
    import ctypes
    import numpy as np
    from incorporating_different_sources_amd import _native
    dev, b, call, where, gammas, R = build(P, k, D, freq, seed=D + k)
    entries = N_PRIOR * N_LEN
    rng = np.random.default_rng(P + R)
    n_patch = int(round(patched * P * R))
    flat = np.sort(rng.choice(P * R, size=n_patch, replace=False))
    patches = (flat // R, (flat % R).astype(np.int32), rng.normal(0.01, 0.05, (n_patch, k)))
    ptr = lambda a, ct: a.ctypes.data_as(ctypes.POINTER(ct))             # noqa: E731

    def download_side(with_patches):
        t0 = time.perf_counter()
        weights = np.empty((R, entries, k))
        dev._check(_native.lib.tp_batch_download_grid_sweep(b._b, ptr(weights, ctypes.c_double), None, None))
        tables = [1.0 / gammas[p] * weights[:, p % entries] if gammas[p] != 1.0 else np.ascontiguousarray(weights[:, p % entries])
                  for p in range(P)]
        if with_patches:
            for q in range(n_patch):
                tables[patches[0][q]][patches[1][q]] = patches[2][q]
        dense = np.concatenate([t.reshape(-1) for t in tables])
        res = dev.replay(weights=dense, w_off=np.arange(P, dtype=np.int64) * R * k, w_stride=np.full(P, k, dtype=np.int64), **call)
        return res, (time.perf_counter() - t0) * 1e3, dev.last_timing()["kernel_ms"]

    def in_place_side(with_patches):
        t0 = time.perf_counter()
        res = b.replay(_native.REPLAY_SRC_GRID_SWEEP, w_scale=1.0 / gammas, patches=patches if with_patches else None, **where, **call)
        return res, (time.perf_counter() - t0) * 1e3, dev.last_timing()["kernel_ms"]

    rec = {"freq": freq, "portfolios": P, "k": k, "days": D, "rebalancing_dates": R, "reps": reps, "patched_pairs": n_patch}
    lines = [f"{freq}: P={P} k={k} days={D} rebalancing dates={R}  sweep results on the device: {R * entries * k * 8 / 2**20:.0f} MiB"]
    for with_patches in (False, True):
        a, _, _ = download_side(with_patches)                              # warm-up of both sides, and the comparison
        c, _, _ = in_place_side(with_patches)
        if not all(x.tobytes() == y.tobytes() for x, y in zip(a, c)):
            raise SystemExit(f"{freq}: the two sides disagree (patches: {with_patches})")
        if (a[3] != 0).any():
            raise SystemExit(f"{freq}: a portfolio tripped the sum check")
        t = {"download": ([], []), "in place": ([], [])}
        for _ in range(reps):
            for name, side in (("download", download_side), ("in place", in_place_side)):
                _, wall, kern = side(with_patches)
                t[name][0].append(wall)
                t[name][1].append(kern)
        tag = f"{n_patch} pairs patched ({patched:.0%})" if with_patches else "unpatched"
        lines.append(f"  {tag}: results equal byte for byte")
        for name in ("download", "in place"):
            wall, kern = t[name]
            lines.append(f"    {name:9s} wall {statistics.median(wall):9.2f} ms [{min(wall):.2f} - {max(wall):.2f}]   "
                         f"kernel {statistics.median(kern):8.3f} ms [{min(kern):.3f} - {max(kern):.3f}]")
            rec[f"{name.replace(' ', '_')}_{'patched' if with_patches else 'unpatched'}"] = {
                "wall_ms": wall, "kernel_ms": kern, "wall_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kern)}
        lines.append(f"    wall download / in place = {statistics.median(t['download'][0]) / statistics.median(t['in place'][0]):.1f}x   "
                     f"kernel in place / download = {statistics.median(t['in place'][1]) / statistics.median(t['download'][1]):.3f}")
    b.close()
    record.append(rec)
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--patched", type=float, default=0.05)
    ap.add_argument("--out", default=None, help="text report; FILE.json next to it holds every repetition")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    record = []
    for freq in args.freqs.split(","):
        measure(args.portfolios, args.k, args.days, freq, args.reps, args.patched, out, record)
    if out:
        out.close()
        with open(args.out + ".json", "a") as f:
            f.write(json.dumps(record) + "\n")


if __name__ == "__main__":
    main()
