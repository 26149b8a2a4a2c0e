#!/usr/bin/env python3
"""Solve sweep against the two-run path of the parent commit, timed with the library's own HIP events.

    python tools/time_solve_sweep.py --parent DIR [--rounds 3] [--out FILE]

DIR is a checkout of the parent commit with its library built (make -C DIR/incorporating_different_sources_amd/csrc).
Every measurement runs in a fresh child process: "old" imports the package of DIR and runs today's path - every date's
index arrays repeated once per draw, two runs (right-hand side t, then 1) - "new" imports this tree and runs one sweep.
Old and new alternate `--rounds` times.  Shapes:

    greyserman  k = 50, 249 rows, 32 dates x 1000 shifts, R = 2, index layout as batch.pack_windows emits it
    jorion      k = 100, 249 rows, W = 10,000, S = 1, R = 2 (BASELINE configs[1], contiguous)
    e2e         calculate_greyserman_portfolio for one date (k = 50, 250-day window), host wall time

kernel_ms is tp_last_timing's kernel span (old: the two runs added), median of `--reps` repetitions after one warm-up;
wall_ms is the host time of one whole repetition, upload and downloads included.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.append(REPO)        # a child started by hand (e.g. under rocprofv3) finds this tree; PYTHONPATH goes first


def greyserman_inputs(np, synthetic, dates=32, k=50, N=250):
    inp = synthetic.make_kernel_inputs(k, N, dates, seed=20250501)
    rng = np.random.default_rng(20250501)
    n_r = inp["n_r"]
    panel = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], 14))], axis=1)
    kw = dict(panel=panel,
              row_idx=(inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32),
              n_rows=np.full(dates, n_r, dtype=np.int32),
              col_idx=np.stack([np.sort(rng.permutation(panel.shape[1])[:k]) for _ in range(dates)]).astype(np.int32),
              rf_adj=rng.normal(0, 1e-4, size=(dates, n_r)))
    eta = rng.gamma(1.0, 10.0, size=(dates, 1000))
    return kw, eta, k, N, n_r


def child(mode, shape, reps):
    import numpy as np
    from incorporating_different_sources_amd import _native, synthetic
    dev = _native.Device(0)
    res = dict(mode=mode, shape=shape, lib=_native.LIB_PATH)

    def two_runs(b, W, k):
        """today's path on an uploaded batch: kernel ms of both runs"""
        b.keep_rhs()
        b.run().download(want_aux=False)
        ms = dev.last_timing()["kernel_ms"]
        b.download_rhs()
        b.keep_rhs(False)
        b.set_rhs(np.ones((W, k)))
        b.run().download(want_aux=False)
        return ms + dev.last_timing()["kernel_ms"]

    if shape == "greyserman":
        kw, eta, k, N, n_r = greyserman_inputs(np, synthetic)
        D, B = eta.shape

        def once():
            t0 = time.perf_counter()
            if mode == "old":
                rep = {key: (np.repeat(val, B, axis=0) if key != "panel" else val) for key, val in kw.items()}
                shift = np.zeros((D * B, 2))
                shift[:, 0] = eta.reshape(-1) / 2
                b = _native.Batch(dev, "jeffreys", k, N, n_r, 1.0, D * B, 0, flags=_native.FLAG_NO_CENTER)
                b.set_shift(shift)
                b.upload(**rep)
                ms = two_runs(b, D * B, k)
            else:
                shift = np.zeros((D, B, 2))
                shift[:, :, 0] = eta / 2
                b = _native.Batch(dev, "jeffreys", k, N, n_r, 1.0, D, 0, flags=_native.FLAG_NO_CENTER)
                b.upload(**kw)
                b.solve_sweep(shift=shift, rhs=np.ones((D, 1, k)))
                ms = dev.last_timing()["kernel_ms"]
                b.download_sweep_rhs()
            b.close()
            return ms, (time.perf_counter() - t0) * 1e3
    elif shape == "jorion":
        c = synthetic.config_shapes(2)
        inp = synthetic.make_kernel_inputs(c["k"], c["N"], c["W"], seed=c["seed"])
        k, N, W = c["k"], c["N"], c["W"]

        def once():
            t0 = time.perf_counter()
            b = _native.Batch(dev, "jeffreys", k, N, inp["n_r"], 1.0, W, 0, flags=_native.FLAG_CENTER_BY_ROWS)
            b.upload(inp["panel"], start=inp["start"])
            if mode == "old":
                ms = two_runs(b, W, k)
            else:
                b.solve_sweep(rhs=np.ones((W, 1, k)))
                ms = dev.last_timing()["kernel_ms"]
                b.download_sweep_rhs()
            b.close()
            return ms, (time.perf_counter() - t0) * 1e3
    else:
        from incorporating_different_sources_amd import portfolio_calculations as pc
        k, N = 50, 250
        inp = synthetic.make_kernel_inputs(k, N, 1, seed=20250502)
        date, prices_df, _, _, rf_df = synthetic.window_frames(inp, 0, [f"T{i:03d}" for i in range(k)])
        spec = {"weighting_strategy": "greyserman", "size": k, "risk_aversion": 5, "turnover_cost": 15,
                "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
                "mcm_scaling": None, "display_name": "greyserman"}

        def once():
            np.random.seed(7)
            t0 = time.perf_counter()
            pc.calculate_greyserman_portfolio(spec, date, prices_df, rf_df)
            return 0.0, (time.perf_counter() - t0) * 1e3

    once()
    runs = [once() for _ in range(reps)]
    res["kernel_ms"] = statistics.median(r[0] for r in runs)
    res["wall_ms"] = statistics.median(r[1] for r in runs)
    res["kernel_ms_all"] = [round(r[0], 4) for r in runs]
    dev.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="greyserman,jorion,e2e")
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=2, metavar=("MODE", "SHAPE"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.reps)
    modes = (["old"] if args.parent else []) + ["new"]
    lines = []
    for shape in args.shapes.split(","):
        rows = {m: [] for m in modes}
        for _ in range(args.rounds):
            for mode in modes:
                tree = os.path.abspath(args.parent) if mode == "old" else REPO
                env = dict(os.environ, PYTHONPATH=tree)
                env.pop("TANGENCY_LIB", None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, shape, "--reps", str(args.reps)],
                                   env=env, cwd=tree, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:          # a failed child ends the measurement: nothing more is started on the device
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit(f"{mode} {shape}: child exited with {p.returncode}")
                rows[mode].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        for i in range(args.rounds):
            parts = [f"{m} kernel {rows[m][i]['kernel_ms']:10.3f} ms  wall {rows[m][i]['wall_ms']:10.1f} ms" for m in modes]
            ratio = ""
            if "old" in rows:
                key = "wall_ms" if shape == "e2e" else "kernel_ms"
                ratio = f"   old/new ({key}) = {rows['old'][i][key] / max(rows['new'][i][key], 1e-9):.2f}"
            lines.append(f"{shape:11s} round {i + 1}: " + "   ".join(parts) + ratio)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
