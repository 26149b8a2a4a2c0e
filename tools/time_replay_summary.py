#!/usr/bin/env python3
"""The device summary of a replay over a grid of trading costs (`Device.replay_summary`, tp_replay_summary) against the path it
replaces, both in one process on one box, on the same portfolios.

    python tools/time_replay_summary.py [--portfolios 256,4096] [--k 100] [--days 2500] [--costs 8] [--reps 5] [--out FILE]

`--portfolios` portfolios of `--k` assets over `--days` trading days, rebalanced monthly, evaluated at `--costs` trading costs.
The portfolios read 256 weight tables round robin (their upload stays small and is the same on both sides) and differ in
universe table, eight to a table.

  "per cost"  what there was before: every cost is a portfolio of its own - ONE tp_replay_run of P x C portfolios at their own
              costs, tp_replay_download of their returns, turnover and metrics, then `summary_records_host` on them;
  "summary"   ONE tp_replay_run of P portfolios at cost 0, nothing downloaded, tp_replay_summary over the C costs,
              tp_replay_download_summary.

Per side: wall ms of the whole call sequence (both include the upload of the same weight tables), kernel ms from the handle's
HIP events (the replay and the summary separately: two steps of one region) and the bytes that cross to the host.  Medians of
`--reps` repetitions after one warm-up of each side, the sides alternated, min - max next to every median.  The records of the
two sides are compared (statuses and counts equal, values to 1e-9) before any time is printed.  One process, one device; run
it under a time limit.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N_TABLES = 256


def build(P, k, D, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    reb_day = np.arange(0, D, 21, dtype=np.int32)
    R = reb_day.size
    K = 5 * k
    n_uni = (P + 7) // 8
    cols = np.stack([np.stack([rng.permutation(K)[:k] for _ in range(R)]) for _ in range(min(n_uni, 64))]).astype(np.int32)
    caps = rng.lognormal(3, 1, cols.shape)
    w = np.abs(rng.normal(0.0, 1.0, (N_TABLES, R, k))) + 0.05
    w /= w.sum(axis=2, keepdims=True)
    port = np.arange(P, dtype=np.int64)
    call = dict(S=rng.normal(0.0004, 0.015, (D, K)), rf_daily=np.full(D, (1 + 0.02) ** (1 / 252) - 1), reb_day=reb_day, K=K,
                weights=w.reshape(-1), cols=cols.reshape(-1), caps=caps.reshape(-1))
    per = dict(k=np.full(P, k, dtype=np.int32), scaling=np.ones(P), w_off=(port % N_TABLES) * R * k,
               w_stride=np.full(P, k, dtype=np.int64), u_off=((port // 8) % cols.shape[0]) * R * k, u_stride=np.full(P, k, dtype=np.int64))
    return call, per, R


def measure(P, k, D, C, reps, out, record):
    import numpy as np
    from incorporating_different_sources_amd import _native, portfolio_evaluation as pe
    call, per, R = build(P, k, D, seed=D + k + P)
    costs = np.linspace(0.0, 35.0, C)
    rf_excess = call["rf_daily"].copy()
    dev = _native.default_device()
    lib = _native.lib

    def per_cost_side():
        t0 = time.perf_counter()
        wide = {name: np.repeat(a, C) for name, a in per.items()}
        ret, turn, _m, status, _bad = dev.replay(cost=np.tile(costs, P), **wide, **call)
        kern = dev.last_timing()["kernel_ms"]
        stats, st = pe.summary_records_host(ret, turn, call["reb_day"], [0.0], rf_excess, replay_status=status)
        return (stats.reshape(P, C, -1), st.reshape(P, C)), (time.perf_counter() - t0) * 1e3, (kern, 0.0)

    def summary_side():
        t0 = time.perf_counter()
        dev._check(lib.tp_region_begin(dev._h))
        dev.replay(cost=np.zeros(P), download=False, **per, **call)
        res = dev.replay_summary(costs, rf_excess)
        total, n, steps = ctypes.c_double(), ctypes.c_int(), (ctypes.c_double * 4)()
        dev._check(lib.tp_region_end(dev._h, ctypes.byref(total)))
        dev._check(lib.tp_region_steps(dev._h, steps, 4, ctypes.byref(n)))
        return res, (time.perf_counter() - t0) * 1e3, (steps[0], steps[1])

    (a, a_st), _, _ = per_cost_side()                                     # warm-up of both sides, and the comparison
    (b, b_st), _, _ = summary_side()
    counts = [0, 1, 2, 10, 12, 13, 18, 19, 27]
    if not (np.array_equal(a_st, b_st) and np.array_equal(a[..., counts], b[..., counts], equal_nan=True)):
        raise SystemExit("the two sides disagree in a status, a day or a count")
    if not (a_st == 0).all():
        raise SystemExit("a record is not TP_SUMMARY_OK")
    if not (np.abs(a - b) <= 1e-9 * np.maximum(1.0, np.abs(a))).all():
        raise SystemExit("the two sides disagree beyond 1e-9")
    t = {"per cost": ([], [], []), "summary": ([], [], [])}
    for _ in range(reps):
        for name, side in (("per cost", per_cost_side), ("summary", summary_side)):
            _, wall, (k_replay, k_summary) = side()
            t[name][0].append(wall)
            t[name][1].append(k_replay)
            t[name][2].append(k_summary)
    down = {"per cost": P * C * ((D + R + 5 * R) * 8 + 8), "summary": P * C * (32 * 8 + 4)}
    tiles = 2 * ((D - 1 + 63) // 64)                                      # two passes over the row
    lines = [f"P={P} k={k} days={D} rebalancing dates={R} costs={C}: records equal in statuses, days and counts, values to 1e-9"]
    rec = {"portfolios": P, "k": k, "days": D, "rebalancing_dates": R, "costs": C, "reps": reps}
    med = statistics.median
    for name in ("per cost", "summary"):
        wall, k_replay, k_summary = t[name]
        lines.append(f"  {name:8s} wall {med(wall):10.2f} ms [{min(wall):.2f} - {max(wall):.2f}]   replay kernel {med(k_replay):8.3f} ms "
                     f"[{min(k_replay):.3f} - {max(k_replay):.3f}]   summary kernel {med(k_summary):7.3f} ms "
                     f"[{min(k_summary):.3f} - {max(k_summary):.3f}]   to the host {down[name] / 2**20:9.2f} MiB")
        rec[name.replace(" ", "_")] = {"wall_ms": wall, "replay_kernel_ms": k_replay, "summary_kernel_ms": k_summary,
                                       "bytes_to_host": down[name]}
    ks = med(t["summary"][2])
    lines.append(f"  wall per cost / summary = {med(t['per cost'][0]) / med(t['summary'][0]):.1f}x   summary kernel: {P * C} waves, "
                 f"{tiles} tiles of 64 days each, {ks * 1e3 / tiles:.2f} us per tile of the launch")
    record.append(rec)
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--portfolios", default="256,4096")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--days", type=int, default=2500)
    ap.add_argument("--costs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="text report; FILE with .json instead of .txt holds every repetition")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    record = []
    for P in args.portfolios.split(","):
        measure(int(P), args.k, args.days, args.costs, args.reps, out, record)
    if out:
        out.close()
        with open(os.path.splitext(args.out)[0] + ".json", "a") as f:
            f.write(json.dumps(record) + "\n")


if __name__ == "__main__":
    main()
