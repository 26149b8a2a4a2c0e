#!/usr/bin/env python3
"""Grid sweep against the two ways a caller has without it, timed with the library's own HIP events.

    python tools/time_grid_sweep.py [--sizes 25,50,75,100] [--dates 1000] [--cases conj1,conj4,jeffreys] [--reps 3] [--out FILE]

Synthetic market data (synthetic.make_market_data: business days, rf = 0.02, so the lengths' risk-free offsets differ and the
sweeps run the delta kernel), daily windows {60, 120, 250, 500}, the index layout batch.pack_windows emits.

  "window sweeps"  per size one batch.pack_windows_lengths, one upload and one Batch.window_sweep   (S packs, S uploads);
  "size sweeps"    per length one batch.pack_windows_nested, one upload and one Batch.size_sweep    (L packs, L uploads);
  "grid sweep"     one batch.pack_windows_grid at (largest size, longest window), one upload, one Batch.grid_sweep.

device ms is tp_last_timing's kernel span (summed over the calls of a way), host ms the wall time of packing and of
upload + call + download; medians of `--reps` repetitions after one warm-up, the three ways alternated inside each repetition.
`--sizes` with 16 entries measures the 16-size build of the fill.  One process, one device; run it under a time limit.
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


def measure(sizes, case, reps, md, dates):
    import numpy as np
    from incorporating_different_sources_amd import _native, batch
    names = CASES[case]
    conj = names[0] != "jeffreys"
    strategy = "conjugate" if conj else "jeffreys"
    dev = _native.default_device()
    W, P, S, L, k = len(dates), len(names), len(sizes), len(WINDOWS), sizes[-1]

    def upload_of(kw):
        return {key: val for key, val in kw.items() if key not in ("n_r", "m")}

    def priors(caps, ks_list, lengths, kk):
        """n0 [W x P x len(lengths)] and w0 [W x P x len(ks_list) x kk] of the case's priors"""
        n0 = np.empty((W, P, len(lengths)))
        w0 = np.zeros((W, P, len(ks_list), kk))
        for p, nm in enumerate(names):
            for l, N in enumerate(lengths):
                n0[:, p, l] = batch.prior_inputs(dates, spec(nm, kk, N), md, caps)[1]
            for s, ks in enumerate(ks_list):
                w0[:, p, s, :ks] = batch.prior_inputs(dates[:1], spec(nm, ks, lengths[-1]), md, caps[:, :ks])[0]
        return n0, w0

    def window_sweeps():
        pack_ms = call_ms = dev_ms = 0.0
        for ks in sizes:
            t0 = time.perf_counter()
            kw, _, caps, rows, delta, mask = batch.pack_windows_lengths(dates, spec(names[0], ks, WINDOWS[-1]), WINDOWS, md)
            n0 = w0 = None
            if conj:
                n0, w0 = priors(caps, [ks], WINDOWS, ks)
                w0 = np.ascontiguousarray(w0[:, :, 0])
            t1 = time.perf_counter()
            b = _native.Batch(dev, strategy, ks, WINDOWS[-1], kw["n_r"], 5.0, W, kw.get("m") or 0)
            b.upload(**upload_of(kw))
            b.window_sweep(WINDOWS, rows, n0, w0, delta=delta if delta.any() else None, want_aux=False)
            dev_ms += dev.last_timing()["kernel_ms"]
            b.close()
            pack_ms += (t1 - t0) * 1e3
            call_ms += (time.perf_counter() - t1) * 1e3
        return dev_ms, pack_ms, call_ms

    def size_sweeps():
        pack_ms = call_ms = dev_ms = 0.0
        for N in WINDOWS:
            t0 = time.perf_counter()
            kw, _, caps, mask = batch.pack_windows_nested(dates, spec(names[0], k, N), sizes, md)
            n0 = w0 = None
            if conj:
                n0, w0 = priors(caps, sizes, [N], k)
                n0 = np.ascontiguousarray(n0[:, :, 0])
            t1 = time.perf_counter()
            b = _native.Batch(dev, strategy, k, N, kw["n_r"], 5.0, W, kw.get("m") or 0)
            b.upload(**upload_of(kw))
            b.size_sweep(sizes, n0, w0, want_aux=False)
            dev_ms += dev.last_timing()["kernel_ms"]
            b.close()
            pack_ms += (t1 - t0) * 1e3
            call_ms += (time.perf_counter() - t1) * 1e3
        return dev_ms, pack_ms, call_ms

    def grid_sweep():
        t0 = time.perf_counter()
        kw, _, caps, rows, delta, mask = batch.pack_windows_grid(dates, spec(names[0], k, WINDOWS[-1]), sizes, WINDOWS, md)
        n0 = w0 = None
        if conj:
            n0, w0 = priors(caps, sizes, WINDOWS, k)
        t1 = time.perf_counter()
        b = _native.Batch(dev, strategy, k, WINDOWS[-1], kw["n_r"], 5.0, W, kw.get("m") or 0)
        b.upload(**upload_of(kw))
        b.grid_sweep(sizes, WINDOWS, rows, n0, w0, delta=delta if delta.any() else None, want_aux=False)
        dev_ms = dev.last_timing()["kernel_ms"]
        b.close()
        assert mask.all() and delta.any()
        return dev_ms, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    ways = (("window sweeps", window_sweeps), ("size sweeps", size_sweeps), ("grid sweep", grid_sweep))
    for _, fn in ways:
        fn()
    runs = {name: [] for name, _ in ways}
    for _ in range(reps):                                   # alternated: every repetition runs the three ways in turn
        for name, fn in ways:
            runs[name].append(fn())
    out = {name: [statistics.median(r[i] for r in rs) for i in range(3)] for name, rs in runs.items()}
    tag = f"S={S:2d} k={k:3d} dates={W:5d} {case:8s}"
    lines = [f"{tag} {name:13s}: device {v[0]:9.3f} ms   pack {v[1]:9.1f} ms   upload+call {v[2]:9.1f} ms" for name, v in out.items()]
    g = out["grid sweep"]
    for name in ("window sweeps", "size sweeps"):
        a = out[name]
        lines.append(f"{tag} {name} / grid sweep: device {a[0] / g[0]:.2f}   host {(a[1] + a[2]) / (g[1] + g[2]):.2f}"
                     f"   (pack {a[1] / g[1]:.2f}, upload+call {a[2] / g[2]:.2f})")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="25,50,75,100")
    ap.add_argument("--dates", type=int, default=1000)
    ap.add_argument("--cases", default="conj1,conj4,jeffreys")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import pandas as pd
    from incorporating_different_sources_amd import batch, synthetic
    sizes = [int(x) for x in args.sizes.split(",")]
    md, _ = synthetic.make_market_data(n_tickers=sizes[-1] + 10, n_days=args.dates + WINDOWS[-1] + 20, seed=20250901)
    days = md["stock_prices_df"].index
    dates = [pd.Timestamp(d) for d in days[WINDOWS[-1] + 10:WINDOWS[-1] + 10 + args.dates]]
    text = []
    for case in args.cases.split(","):
        lines = measure(sizes, case, args.reps, md, dates)
        print("\n".join(lines), flush=True)
        text += lines
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(text) + "\n")
    batch.clear_panel_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
