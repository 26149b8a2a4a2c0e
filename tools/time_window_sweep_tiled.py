#!/usr/bin/env python3
"""Tiled window sweep (k > sweep_max_assets()) against what a caller does without it, timed with the library's own HIP events.

    python tools/time_window_sweep_tiled.py [--shapes k500,k1000] [--cases conj1,conj4,jeffreys] [--lists short,long] [--reps 3] [--out FILE]

Synthetic returns (synthetic.make_kernel_inputs) in the index layout batch.pack_windows emits (row_idx, n_rows, col_idx, rf_adj
over panels with 14 spare columns), W windows that each hold the rows of the longest length; four lengths per list:

    k500    k = 500,  W = 256, 5 intraday days (m = 389);   short 125 / 250 / 500 / 1000     long 560 / 640 / 800 / 1000
    k1000   k = 1000, W = 64, 22 intraday days (m = 1715);  short 250 / 500 / 1000 / 2000    long 1100 / 1300 / 1600 / 2000

Every N of a "long" list exceeds k, so Jeffreys is well-posed on it; Jeffreys is not run on the short lists.

  "per length"  the way without the sweep: per length the suffix rows cut out on the host, one upload and one tiled batch - a
                plain run for one prior or for Jeffreys, one Batch.prior_sweep_tiled for four priors;
  "sweep"       one upload at the longest window, one Batch.window_sweep_tiled with a delta (the lengths' risk-free offsets
                differ on real calendars, so the delta kernel runs).

device ms is tp_last_timing's kernel span (per length: summed over the lengths), host ms the wall time of cutting, upload,
call and download; medians of `--reps` repetitions after one warm-up.  One process, one device; run it under a time limit.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# k, W, intraday days, {list: lengths}
SHAPES = {"k500": (500, 256, 5, {"short": [125, 250, 500, 1000], "long": [560, 640, 800, 1000]}),
          "k1000": (1000, 64, 22, {"short": [250, 500, 1000, 2000], "long": [1100, 1300, 1600, 2000]})}
PRIORS = {"conj1": 1, "conj4": 4, "jeffreys": 1}


def measure(shape, case, which, reps):
    import numpy as np
    from incorporating_different_sources_amd import _native, synthetic
    k, W, hf_days, lists = SHAPES[shape]
    lengths = lists[which]
    conj = case != "jeffreys"
    P = PRIORS[case]
    strategy = "conjugate" if conj else "jeffreys"
    N = lengths[-1]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=20251001, hf_days=hf_days)
    rng = np.random.default_rng(20251001)
    n_r, m, extra = inp["n_r"], inp["m"], 14
    panel = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], extra))], axis=1)
    hf_panel = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], extra))], axis=1)
    row_idx = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    col_idx = np.stack([rng.permutation(k + extra)[:k] for _ in range(W)]).astype(np.int32)
    rf_adj = rng.normal(0, 1e-4, size=(W, n_r))
    L = len(lengths)
    rows = np.tile(np.asarray([n - 1 for n in lengths], dtype=np.int32), (W, 1))
    delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))
    n0 = np.asarray(lengths)[None, None, :] * np.array([1, 5])[(np.arange(P) // 2) % 2][None, :, None] * rng.uniform(1.0, 1.6, size=(W, P, L))
    caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
    vw = caps / caps.sum(axis=1, keepdims=True)
    w0 = np.ascontiguousarray(np.where((np.arange(P) % 2 == 1)[None, :, None], vw[:, None, :], 1.0 / k))
    hf = dict(hf_panel=hf_panel, hf_start=inp["hf_start"]) if conj else {}
    dev = _native.default_device()

    def per_length():
        t0 = time.perf_counter()
        dev_ms = 0.0
        for l, n in enumerate(lengths):
            r = n - 1
            b = _native.Batch(dev, strategy, k, n, r, 5.0, W, m if conj else 0)
            pri = dict(w0=np.ascontiguousarray(w0[:, 0]), n0=np.ascontiguousarray(n0[:, 0, l])) if conj else {}
            b.upload(panel, row_idx=np.ascontiguousarray(row_idx[:, n_r - r:]), n_rows=np.full(W, r, dtype=np.int32), col_idx=col_idx,
                     rf_adj=np.ascontiguousarray(rf_adj[:, n_r - r:] + delta[:, l, n_r - r:]), **hf, **pri)
            if P > 1:
                b.prior_sweep_tiled(np.ascontiguousarray(n0[:, :, l]), w0, want_aux=False)
            else:
                b.run().download(want_aux=False)
            dev_ms += dev.last_timing()["kernel_ms"]
            b.close()
        return dev_ms, (time.perf_counter() - t0) * 1e3

    def sweep():
        t0 = time.perf_counter()
        b = _native.Batch(dev, strategy, k, N, n_r, 5.0, W, m if conj else 0)
        pri = dict(w0=np.ascontiguousarray(w0[:, 0]), n0=np.ascontiguousarray(n0[:, 0, -1])) if conj else {}
        b.upload(panel, row_idx=row_idx, n_rows=np.full(W, n_r, dtype=np.int32), col_idx=col_idx, rf_adj=rf_adj, **hf, **pri)
        if conj:
            b.window_sweep_tiled(lengths, rows, n0, w0, delta=delta, want_aux=False)
        else:
            b.window_sweep_tiled(lengths, rows, delta=delta, want_aux=False)
        dev_ms = dev.last_timing()["kernel_ms"]
        b.close()
        return dev_ms, (time.perf_counter() - t0) * 1e3

    out = {}
    for name, fn in (("per length", per_length), ("sweep", sweep)):
        fn()
        runs = [fn() for _ in range(reps)]
        out[name] = [statistics.median(r[i] for r in runs) for i in range(2)]
    a, s = out["per length"], out["sweep"]
    tag = f"{shape:5s} W={W:4d} {case:8s} {which:5s}"
    lines = [f"{tag} {name:10s}: device {v[0]:10.3f} ms   host {v[1]:10.1f} ms" for name, v in out.items()]
    lines.append(f"{tag} per length / sweep: device {a[0] / s[0]:.2f}   host {a[1] / s[1]:.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="k500,k1000")
    ap.add_argument("--cases", default="conj1,conj4,jeffreys")
    ap.add_argument("--lists", default="short,long")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    text = []
    for shape in args.shapes.split(","):
        for case in args.cases.split(","):
            for which in args.lists.split(","):
                if case == "jeffreys" and which == "short":
                    continue                                   # N <= k: not positive definite
                lines = measure(shape, case, which, args.reps)
                print("\n".join(lines), flush=True)
                text += lines
                if args.out:
                    with open(args.out, "w") as f:
                        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
