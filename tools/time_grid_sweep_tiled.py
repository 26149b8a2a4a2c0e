#!/usr/bin/env python3
"""Tiled grid sweep (k > sweep_max_assets()) against the two ways a caller has without it, timed with the library's own HIP events.

    python tools/time_grid_sweep_tiled.py [--shapes k500,k1000,k500s] [--cases conj1,conj4,jeffreys] [--reps 3] [--out FILE]

Synthetic returns (synthetic.make_kernel_inputs) in the index layout batch.pack_windows_grid emits (row_idx, n_rows, col_idx,
rf_adj over panels with 14 spare columns), W windows that each hold the rows of the longest length at the largest size, with a
delta (the lengths' risk-free offsets differ on real calendars, so the delta kernel runs); four sizes x four lengths:

    k500    k = 500,  W = 256, 5 intraday days (m = 389);   sizes 200 / 300 / 400 / 500     lengths 560 / 640 / 800 / 1000
    k1000   k = 1000, W = 64, 22 intraday days (m = 1715);  sizes 250 / 500 / 750 / 1000    lengths 1100 / 1300 / 1600 / 2000
    k500s   k500 at W = 4: W x P <= 16 entries per length - where one group over all lengths shows against groups of one length

Every length exceeds the largest size, so Jeffreys is well-posed on it.

  "per size"    one upload at that size's prefix columns and one Batch.window_sweep_tiled per size;
  "per length"  per length the suffix rows cut out on the host (the delta folded into rf_adj), one upload and one
                Batch.size_sweep_tiled;
  "grid"        one upload at (largest size, longest window) and one Batch.grid_sweep_tiled.

device ms is tp_last_timing's kernel span (summed over the sizes / lengths), host ms the wall time of cutting, upload, call and
download; medians of `--reps` rounds after one warm-up round, the three ways alternated inside a round.  One process, one
device; run it under a time limit.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# k, W, intraday days, sizes, lengths
SHAPES = {"k500": (500, 256, 5, [200, 300, 400, 500], [560, 640, 800, 1000]),
          "k1000": (1000, 64, 22, [250, 500, 750, 1000], [1100, 1300, 1600, 2000]),
          "k500s": (500, 4, 5, [200, 300, 400, 500], [560, 640, 800, 1000])}
PRIORS = {"conj1": 1, "conj4": 4, "jeffreys": 1}


def measure(shape, case, reps):
    import numpy as np
    from incorporating_different_sources_amd import _native, synthetic
    k, W, hf_days, sizes, lengths = SHAPES[shape]
    conj = case != "jeffreys"
    P = PRIORS[case]
    strategy = "conjugate" if conj else "jeffreys"
    N = lengths[-1]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=20251101, hf_days=hf_days)
    rng = np.random.default_rng(20251101)
    n_r, m, extra = inp["n_r"], inp["m"], 14
    panel = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], extra))], axis=1)
    hf_panel = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], extra))], axis=1)
    row_idx = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    col_idx = np.stack([rng.permutation(k + extra)[:k] for _ in range(W)]).astype(np.int32)
    rf_adj = rng.normal(0, 1e-4, size=(W, n_r))
    L, S = len(lengths), len(sizes)
    rows = np.tile(np.asarray([n - 1 for n in lengths], dtype=np.int32), (W, 1))
    delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))
    n0 = np.asarray(lengths)[None, None, :] * np.array([1, 5])[(np.arange(P) // 2) % 2][None, :, None] * rng.uniform(1.0, 1.6, size=(W, P, L))
    caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
    w0 = np.zeros((W, P, S, k))
    for s, ks in enumerate(sizes):
        vw = caps[:, :ks] / caps[:, :ks].sum(axis=1, keepdims=True)
        w0[:, :, s, :ks] = np.where((np.arange(P) % 2 == 1)[None, :, None], vw[:, None, :], 1.0 / ks)
    hf = dict(hf_panel=hf_panel, hf_start=inp["hf_start"]) if conj else {}
    dev = _native.default_device()

    def per_size():
        t0 = time.perf_counter()
        dev_ms = 0.0
        for s, ks in enumerate(sizes):
            b = _native.Batch(dev, strategy, ks, N, n_r, 5.0, W, m if conj else 0)
            pri = dict(w0=np.ascontiguousarray(w0[:, 0, s, :ks]), n0=np.ascontiguousarray(n0[:, 0, -1])) if conj else {}
            b.upload(panel, row_idx=row_idx, n_rows=np.full(W, n_r, dtype=np.int32), col_idx=np.ascontiguousarray(col_idx[:, :ks]),
                     rf_adj=rf_adj, **hf, **pri)
            if conj:
                b.window_sweep_tiled(lengths, rows, n0, np.ascontiguousarray(w0[:, :, s, :ks]), delta=delta, want_aux=False)
            else:
                b.window_sweep_tiled(lengths, rows, delta=delta, want_aux=False)
            dev_ms += dev.last_timing()["kernel_ms"]
            b.close()
        return dev_ms, (time.perf_counter() - t0) * 1e3

    def per_length():
        t0 = time.perf_counter()
        dev_ms = 0.0
        for l, n in enumerate(lengths):
            r = n - 1
            b = _native.Batch(dev, strategy, k, n, r, 5.0, W, m if conj else 0)
            pri = dict(w0=np.ascontiguousarray(w0[:, 0, -1]), n0=np.ascontiguousarray(n0[:, 0, l])) if conj else {}
            b.upload(panel, row_idx=np.ascontiguousarray(row_idx[:, n_r - r:]), n_rows=np.full(W, r, dtype=np.int32), col_idx=col_idx,
                     rf_adj=np.ascontiguousarray(rf_adj[:, n_r - r:] + delta[:, l, n_r - r:]), **hf, **pri)
            if conj:
                b.size_sweep_tiled(sizes, np.ascontiguousarray(n0[:, :, l]), w0, want_aux=False)
            else:
                b.size_sweep_tiled(sizes, want_aux=False)
            dev_ms += dev.last_timing()["kernel_ms"]
            b.close()
        return dev_ms, (time.perf_counter() - t0) * 1e3

    def grid():
        t0 = time.perf_counter()
        b = _native.Batch(dev, strategy, k, N, n_r, 5.0, W, m if conj else 0)
        pri = dict(w0=np.ascontiguousarray(w0[:, 0, -1]), n0=np.ascontiguousarray(n0[:, 0, -1])) if conj else {}
        b.upload(panel, row_idx=row_idx, n_rows=np.full(W, n_r, dtype=np.int32), col_idx=col_idx, rf_adj=rf_adj, **hf, **pri)
        if conj:
            b.grid_sweep_tiled(sizes, lengths, rows, n0, w0, delta=delta, want_aux=False)
        else:
            b.grid_sweep_tiled(sizes, lengths, rows, delta=delta, want_aux=False)
        dev_ms = dev.last_timing()["kernel_ms"]
        b.close()
        return dev_ms, (time.perf_counter() - t0) * 1e3

    ways = (("per size", per_size), ("per length", per_length), ("grid", grid))
    runs = {name: [] for name, _ in ways}
    for rep in range(reps + 1):                                # round 0 warms up; the ways alternate inside a round
        for name, fn in ways:
            res = fn()
            if rep:
                runs[name].append(res)
    out = {name: [statistics.median(r[i] for r in rs) for i in range(2)] for name, rs in runs.items()}
    g = out["grid"]
    tag = f"{shape:5s} W={W:4d} {case:8s}"
    lines = [f"{tag} {name:10s}: device {v[0]:10.3f} ms   host {v[1]:10.1f} ms" for name, v in out.items()]
    for name in ("per size", "per length"):
        lines.append(f"{tag} {name} / grid: device {out[name][0] / g[0]:.2f}   host {out[name][1] / g[1]:.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="k500,k1000,k500s")
    ap.add_argument("--cases", default="conj1,conj4,jeffreys")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="append the lines to this file")
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        for case in args.cases.split(","):
            lines = measure(shape, case, args.reps)
            print("\n".join(lines), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
