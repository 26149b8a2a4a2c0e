#!/usr/bin/env python3
"""Window sweep against what a caller does without it, timed with the library's own HIP events.

    python tools/time_window_sweep.py [--k 50,100] [--dates 1000,10000] [--cases conj1,conj4,jeffreys] [--reps 3] [--out FILE]

Synthetic market data (synthetic.make_market_data: business days, rf = 0.02, so the lengths' risk-free offsets differ and the
sweep runs its delta kernel), daily windows {60, 120, 250, 500}, the index layout batch.pack_windows emits.

  "per length"  the way without the sweep: per window length one batch.pack_windows, one upload and one batch - a plain run for
                one prior or for Jeffreys, one prior sweep (Batch.prior_sweep) for four priors;
  "sweep"       one batch.pack_windows_lengths at the longest window, one upload, one Batch.window_sweep.

device ms is tp_last_timing's kernel span (per length: summed over the lengths), host ms the wall time of packing and of
upload + call + download; medians of `--reps` repetitions after one warm-up.  One process, one device; run it under a time
limit.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

WINDOWS = [60, 120, 250, 500]
CASES = {"conj1": ["conjugate_hf_vix_vw"],
         "conj4": ["conjugate_hf_vix_vw", "conjugate_hf_vix_ew", "conjugate_hf_epu_vw", "conjugate_hf_epu_ew"],
         "jeffreys": ["jeffreys"]}


def spec(strat, k, N):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": "daily",
            "rolling_window": N, "rolling_window_frequency": "daily", "mcm_scaling": 1, "display_name": strat}


def measure(k, n_dates, case, reps, md, dates):
    import numpy as np
    from incorporating_different_sources_amd import _native, batch
    names = CASES[case]
    conj = names[0] != "jeffreys"
    strategy = "conjugate" if conj else "jeffreys"
    dev = _native.default_device()
    W = len(dates)

    def upload_of(kw):
        return {key: val for key, val in kw.items() if key not in ("n_r", "m")}

    def per_length():
        pack_ms = call_ms = dev_ms = 0.0
        for N in WINDOWS:
            t0 = time.perf_counter()
            kw, _, caps = batch.pack_windows(dates, spec(names[0], k, N), md, return_caps=True)
            pri = [batch.prior_inputs(dates, spec(nm, k, N), md, caps) for nm in names[1:]]
            t1 = time.perf_counter()
            b = _native.Batch(dev, strategy, k, N, kw["n_r"], 5.0, W, kw.get("m") or 0)
            b.upload(**upload_of(kw))
            if len(names) > 1:
                b.prior_sweep(np.stack([kw["n0"]] + [p[1] for p in pri], axis=1), np.stack([kw["w0"]] + [p[0] for p in pri], axis=1),
                              want_aux=False)
            else:
                b.run().download(want_aux=False)
            dev_ms += dev.last_timing()["kernel_ms"]
            b.close()
            pack_ms += (t1 - t0) * 1e3
            call_ms += (time.perf_counter() - t1) * 1e3
        return dev_ms, pack_ms, call_ms

    def sweep():
        t0 = time.perf_counter()
        kw, _, caps, rows, delta, mask = batch.pack_windows_lengths(dates, spec(names[0], k, WINDOWS[-1]), WINDOWS, md)
        n0 = w0 = None
        if conj:
            n0 = np.empty((W, len(names), len(WINDOWS)))
            w0 = np.empty((W, len(names), k))
            for p, nm in enumerate(names):
                for l, N in enumerate(WINDOWS):
                    w0[:, p], n0[:, p, l] = batch.prior_inputs(dates, spec(nm, k, N), md, caps)
        t1 = time.perf_counter()
        b = _native.Batch(dev, strategy, k, WINDOWS[-1], kw["n_r"], 5.0, W, kw.get("m") or 0)
        b.upload(**upload_of(kw))
        b.window_sweep(WINDOWS, rows, n0, w0, delta=delta if delta.any() else None, want_aux=False)
        dev_ms = dev.last_timing()["kernel_ms"]
        b.close()
        assert mask.all() and delta.any()
        return dev_ms, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    out = {}
    for name, fn in (("per length", per_length), ("sweep", sweep)):
        fn()
        runs = [fn() for _ in range(reps)]
        out[name] = [statistics.median(r[i] for r in runs) for i in range(3)]
    a, b = out["per length"], out["sweep"]
    lines = [f"k={k:3d} dates={n_dates:6d} {case:8s} {name:10s}: device {v[0]:9.3f} ms   pack {v[1]:9.1f} ms   upload+call {v[2]:9.1f} ms"
             for name, v in out.items()]
    lines.append(f"k={k:3d} dates={n_dates:6d} {case:8s} per length / sweep: device {a[0] / b[0]:.2f}   host {(a[1] + a[2]) / (b[1] + b[2]):.2f}"
                 f"   (pack {a[1] / b[1]:.2f}, upload+call {a[2] / b[2]:.2f})")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", default="50,100")
    ap.add_argument("--dates", default="1000,10000")
    ap.add_argument("--cases", default="conj1,conj4,jeffreys")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import pandas as pd
    from incorporating_different_sources_amd import batch, synthetic
    text = []
    for k in (int(x) for x in args.k.split(",")):
        for n_dates in (int(x) for x in args.dates.split(",")):
            md, _ = synthetic.make_market_data(n_tickers=k + 10, n_days=n_dates + WINDOWS[-1] + 20, seed=20250901)
            days = md["stock_prices_df"].index
            dates = [pd.Timestamp(d) for d in days[WINDOWS[-1] + 10:WINDOWS[-1] + 10 + n_dates]]
            for case in args.cases.split(","):
                lines = measure(k, n_dates, case, args.reps, md, dates)
                print("\n".join(lines), flush=True)
                text += lines
                if args.out:
                    with open(args.out, "w") as f:
                        f.write("\n".join(text) + "\n")
            batch.clear_panel_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
