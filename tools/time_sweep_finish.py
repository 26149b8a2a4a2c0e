#!/usr/bin/env python3
"""The device finish of the Greyserman weights (`Batch.sweep_finish`, tp_batch_sweep_finish) against the path it replaces, both in
one process on one box, on the same windows and the same draws.

    python tools/time_sweep_finish.py [--shapes 50x32,50x1342,500x32] [--draws 1000] [--rows 249] [--reps 5] [--out FILE]

A shape is k x dates; above `sweep_max_assets()` it runs with GREYSERMAN_TILED_SWEEP (one tiled solve sweep per group of dates).
Both sides are `portfolio_calculations._greyserman_batch` on one pack of rolling windows with fixed draws:

  "host"    GREYSERMAN_DEVICE_FINISH off: the solve sweep, the download of its dates x draws x 2 x k solutions,
            `_greyserman_from_solves` in numpy;
  "device"  the flag on: the same sweep with its solutions left on the device, `Batch.sweep_finish`, the download of [dates x k].

Per side: wall ms of the whole call (upload, sweep, finish, download; both upload the same panel) and kernel ms of the handle's
last timed span (host side: the sweep; device side: the finish's two launches).  Medians of `--reps` repetitions after one
warm-up of each side, the sides alternated, min - max next to every median.  The weights of the two sides are compared (to
1e-9 of the largest weight) before any time is printed.  Derivable without a run, printed next to the times: the bytes that
cross to the host drop from 16 W S k to 8 W k, and the finish reads 16 W S k bytes of HBM once.  One process, one device; run
it under a time limit.
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
    kw = dict(panel=panel, start=np.arange(W, dtype=np.int64), n_r=n_r, n_rows=np.full(W, n_r, dtype=np.int32))
    draws = (rng.uniform(-1000, 1000, size=(W, S)), rng.standard_gamma(1.0, size=(W, S)) * 10)
    tiled = k > _native.sweep_max_assets()
    dev = _native.default_device()

    def side(flag):
        pc.GREYSERMAN_DEVICE_FINISH = flag
        pc.GREYSERMAN_TILED_SWEEP = tiled
        try:
            t0 = time.perf_counter()
            w = pc._greyserman_batch(kw, 5.0, k, n_r + 1, draws=draws)
            return w, (time.perf_counter() - t0) * 1e3, dev.last_timing()["kernel_ms"]
        finally:
            pc.GREYSERMAN_DEVICE_FINISH = False
            pc.GREYSERMAN_TILED_SWEEP = False

    a, _, _ = side(False)                                                 # warm-up of both sides, and the comparison
    b, _, _ = side(True)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise SystemExit("a weight is not finite")
    if not (np.abs(a - b).max(axis=1) <= 1e-9 * np.abs(a).max(axis=1)).all():
        raise SystemExit("the two sides disagree beyond 1e-9 of a date's largest weight")
    t = {"host": ([], []), "device": ([], [])}
    for _ in range(reps):
        for name, flag in (("host", False), ("device", True)):
            _, wall, kern = side(flag)
            t[name][0].append(wall)
            t[name][1].append(kern)
    down = {"host": 16 * W * S * k, "device": 8 * W * k}
    med = statistics.median
    lines = [f"k={k}{' (tiled sweep)' if tiled else ''} dates={W} draws={S} rows={n_r}: weights equal to 1e-9 of each date's largest; "
             f"the finish reads {16 * W * S * k / 2**20:.1f} MiB of HBM once"]
    rec = {"k": k, "dates": W, "draws": S, "rows": n_r, "tiled": tiled, "reps": reps}
    for name, what in (("host", "sweep kernels"), ("device", "finish kernels")):
        wall, kern = t[name]
        lines.append(f"  {name:6s} wall {med(wall):10.2f} ms [{min(wall):.2f} - {max(wall):.2f}]   {what} {med(kern):9.3f} ms "
                     f"[{min(kern):.3f} - {max(kern):.3f}]   to the host {down[name] / 2**20:10.3f} MiB")
        rec[name] = {"wall_ms": wall, "last_kernel_ms": kern, "bytes_to_host": down[name]}
    lines.append(f"  wall host / device = {med(t['host'][0]) / med(t['device'][0]):.2f}x")
    record.append(rec)
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="50x32,50x1342,500x32", help="k x dates, comma separated")
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
