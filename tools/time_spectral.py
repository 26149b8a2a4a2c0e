#!/usr/bin/env python3
"""The spectral ridge sweep (`Batch.spectral_greyserman`, tp_batch_spectral_greyserman: one eigendecomposition per date) against
the path it is an alternative to (`Batch.solve_sweep(download=False)` + `Batch.sweep_finish`: one factorisation per draw), both
in one process on one box, on the same uploaded batch and the same draws.

    python tools/time_spectral.py [--shapes 50x32,50x1342,143x469] [--draws 1000] [--rows 249] [--reps 5] [--out FILE]

A shape is k x dates, k <= `sweep_max_assets()`.  Per side and repetition, after one warm-up of each side and with the sides
alternated:
  wall ms    from the first call to the [dates x k] weights and statuses on the host (the upload is shared and not counted);
  kernel ms  the steps of a `region_begin` / `region_end` bracket: "finish" has two (the sweep with its Gram pass, the finish),
             "spectral" one (Gram pass, eigensolver, group and window kernels).
The eigensolver does not depend on the draws, so one more timed spectral call with ONE draw per date gives the split: that
call is the Gram pass, the eigendecompositions and the product with V; the difference to the full call is what the draws cost.
Medians of `--reps`, min - max next to every median; the Jacobi sweep counts of the dates (min / median / max) are printed too.
The weights of the two sides are compared (to 1e-9 of each date's largest weight) before any time is printed.  One process, one
device; run it under a time limit.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def measure(k, W, S, n_r, reps, out, record):
    import numpy as np
    from incorporating_different_sources_amd import _native, portfolio_calculations as pc
    rng = np.random.Generator(np.random.PCG64(k * 100003 + W))
    beta = rng.uniform(0.5, 1.5, size=k)
    f = rng.normal(0.0, 0.01, size=W + n_r)
    panel = np.ascontiguousarray(3e-4 + f[:, None] * beta[None, :] + rng.normal(0.0, 0.01, size=(W + n_r, k)))
    xi, eta = rng.uniform(-1000, 1000, size=(W, S)), rng.standard_gamma(1.0, size=(W, S)) * 10
    n = np.full(W, float(n_r))
    kappa = pc._greyserman_kappa(n)
    shift = np.zeros((W, S, 2))
    shift[:, :, 0] = eta / 2
    ones = np.ones((W, 1, k))
    dev = _native.default_device()
    med = statistics.median

    with _native.Batch(dev, "jeffreys", k, n_r + 1, n_r, 1.0, W, 0, flags=_native.FLAG_NO_CENTER) as b:
        b.upload(panel, start=np.arange(W, dtype=np.int64))

        def finish():
            dev.region_begin()
            t0 = time.perf_counter()
            b.solve_sweep(shift=shift, rhs=ones, default_rhs=True, download=False)
            b.sweep_finish(_native.FINISH_GREYSERMAN, n, 5.0, kappa=kappa, xi=xi, eta=eta)
            w, status, _ = b.download_sweep_finish()
            wall = (time.perf_counter() - t0) * 1e3
            dev.region_end()
            return w, status, wall, list(dev.region_steps())

        def spectral(draws=S):
            dev.region_begin()
            t0 = time.perf_counter()
            b.spectral_greyserman(n, 5.0, kappa, xi[:, :draws], eta[:, :draws])
            w, status, _ = b.download_spectral()
            wall = (time.perf_counter() - t0) * 1e3
            dev.region_end()
            return w, status, wall, list(dev.region_steps())

        a, sa, _, _ = finish()                                # warm-up of both sides, and the comparison
        c, sc, _, _ = spectral()
        if (sa != 0).any() or (sc != 0).any():
            raise SystemExit(f"statuses: finish {sorted(set(sa.tolist()))}, spectral {sorted(set(sc.tolist()))}")
        if not (np.abs(a - c).max(axis=1) <= 1e-9 * np.abs(a).max(axis=1)).all():
            raise SystemExit("the two sides disagree beyond 1e-9 of a date's largest weight")
        sweeps = b.download_spectral(want_spectrum=True)[4]
        spectral(1)
        t = {"finish": [], "spectral": [], "spectral, 1 draw": []}
        for _ in range(reps):
            for name, call in (("finish", finish), ("spectral", spectral), ("spectral, 1 draw", lambda: spectral(1))):
                _, _, wall, steps = call()
                t[name].append((wall, steps))

    lines = [f"k={k} dates={W} draws={S} rows={n_r}: weights equal to 1e-9 of each date's largest; Jacobi sweeps "
             f"min / median / max = {int(sweeps.min())} / {int(med(sweeps.tolist()))} / {int(sweeps.max())}"]
    rec = {"k": k, "dates": W, "draws": S, "rows": n_r, "reps": reps, "sweeps": [int(sweeps.min()), int(med(sweeps.tolist())), int(sweeps.max())]}
    kern = {}
    for name, runs in t.items():
        wall = [r[0] for r in runs]
        total = [sum(r[1]) for r in runs]
        kern[name] = med(total)
        steps = " + ".join(f"{med([r[1][i] for r in runs]):.3f}" for i in range(len(runs[0][1])))
        lines.append(f"  {name:17s} wall {med(wall):10.2f} ms [{min(wall):.2f} - {max(wall):.2f}]   kernels {med(total):10.3f} ms "
                     f"[{min(total):.3f} - {max(total):.3f}]" + (f"   = {steps}" if len(runs[0][1]) > 1 else ""))
        rec[name] = {"wall_ms": wall, "step_ms": [r[1] for r in runs]}
    lines.append(f"  kernels finish / spectral = {kern['finish'] / kern['spectral']:.2f}x   wall finish / spectral = "
                 f"{med([r[0] for r in t['finish']]) / med([r[0] for r in t['spectral']]):.2f}x   spectral: Gram + eigensolver + V "
                 f"product {kern['spectral, 1 draw']:.3f} ms, the draws {kern['spectral'] - kern['spectral, 1 draw']:.3f} ms")
    record.append(rec)
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="50x32,50x1342,143x469", help="k x dates, comma separated")
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=249)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="text report; FILE with .json instead of .txt holds every repetition")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    record = []
    for shape in args.shapes.split(","):
        k, W = (int(v) for v in shape.split("x"))
        measure(k, W, args.draws, args.rows, args.reps, out, record)
    if out:
        out.close()
        with open(os.path.splitext(args.out)[0] + ".json", "a") as f:
            f.write(json.dumps(record) + "\n")


if __name__ == "__main__":
    main()
