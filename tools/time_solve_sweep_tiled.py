#!/usr/bin/env python3
"""Large-k (tiled) solve sweep against the replicated two-run batch of the parent commit, timed with the library's own HIP events.

    python tools/time_solve_sweep_tiled.py --parent DIR [--rounds 3] [--out FILE]

DIR is a checkout of the parent commit with its library built (make -C DIR/incorporating_different_sources_amd/csrc).
Every measurement runs in a fresh child process under a `timeout` of its own: "old" imports the package of DIR and runs what
_greyserman_batch_repeated does there - every window's index arrays repeated once per shift, ONE batch of S x W windows, two
launches (right-hand side t with keep_rhs, then set_rhs(1)) - "new" imports this tree, uploads the W windows once and runs one
tiled solve sweep (Batch.solve_sweep_tiled, R = 2: t and 1).  Old and new alternate `--rounds` times.  Shapes:

    g200   k = 200, 249 daily rows, index layout as batch.pack_windows emits it, 32 dates x 1,000 shifts (Greyserman)
    g500   the same at k = 500
    j500   k = 500, W = 4,096, contiguous, S = 1, no shift (Jorion's V^-1 [mu, 1]: expected to lose - nothing is shared)

kernel_ms is tp_last_timing's kernel span (old: the sum of its two launches), median of `--reps` repetitions after one
warm-up; wall_ms is the host time of one whole repetition, index replication, batch creation, upload and downloads included.
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

# (k, N, W, S, index layout)
SHAPES = {"g200": (200, 250, 32, 1000, True), "g500": (500, 250, 32, 1000, True), "j500": (500, 250, 4096, 1, False)}


def inputs(np, synthetic, k, N, W, S, index):
    inp = synthetic.make_kernel_inputs(k, N, W, seed=20251001)
    rng = np.random.default_rng(20251001)
    n_r = inp["n_r"]
    kw = dict(panel=inp["panel"], start=inp["start"])
    if index:
        extra = 14
        kw["panel"] = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], extra))], axis=1)
        del kw["start"]
        kw.update(row_idx=(inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32),
                  n_rows=np.full(W, n_r, dtype=np.int32),
                  col_idx=np.stack([np.sort(rng.permutation(k + extra)[:k]) for _ in range(W)]).astype(np.int32),
                  rf_adj=rng.normal(0, 1e-4, size=(W, n_r)))
    shift = None
    if S > 1:
        shift = np.zeros((W, S, 2))
        shift[:, :, 0] = rng.gamma(1.0, 10.0, size=(W, S)) / 2          # eta_b / 2
    return kw, shift, n_r


def child(mode, shape, reps):
    import numpy as np
    from incorporating_different_sources_amd import _native, synthetic
    k, N, W, S, index = SHAPES[shape]
    kw, shift, n_r = inputs(np, synthetic, k, N, W, S, index)
    dev = _native.Device(0)
    res = dict(mode=mode, shape=shape, lib=_native.LIB_PATH)
    per_window = ("start", "row_idx", "n_rows", "col_idx", "rf_adj")

    def once():
        t0 = time.perf_counter()
        if mode == "old":
            big = {key: (np.repeat(np.asarray(val), S, axis=0) if key in per_window else val) for key, val in kw.items()}
            b = _native.Batch(dev, "jeffreys", k, N, n_r, 1.0, W * S, 0, flags=_native.FLAG_NO_CENTER)
            if shift is not None:
                b.set_shift(shift.reshape(W * S, 2))
            b.upload(**big)
            b.keep_rhs()
            b.run().download(want_aux=False)
            ms = dev.last_timing()["kernel_ms"]
            b.download_rhs()
            b.keep_rhs(False)
            b.set_rhs(np.ones((W * S, k)))
            b.run().download(want_aux=False)
            ms += dev.last_timing()["kernel_ms"]
        else:
            b = _native.Batch(dev, "jeffreys", k, N, n_r, 1.0, W, 0, flags=_native.FLAG_NO_CENTER)
            b.upload(**kw)
            b.solve_sweep_tiled(shift=shift, rhs=np.ones((W, 1, k)), default_rhs=True)
            ms = dev.last_timing()["kernel_ms"]
            b.download_sweep_rhs()
        b.close()
        return ms, (time.perf_counter() - t0) * 1e3

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
    ap.add_argument("--shapes", default="g200,g500,j500")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one measurement may take")
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
                p = subprocess.run(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__),
                                    "--child", mode, shape, "--reps", str(args.reps)],
                                   env=env, cwd=tree, capture_output=True, text=True)
                if p.returncode != 0:          # a failed child ends the measurement: nothing more is started on the device
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit(f"{mode} {shape}: child exited with {p.returncode}")
                rows[mode].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        for i in range(args.rounds):
            parts = [f"{m} kernel {rows[m][i]['kernel_ms']:10.3f} ms  wall {rows[m][i]['wall_ms']:10.1f} ms" for m in modes]
            ratio = ""
            if "old" in rows:
                ratio = (f"   old/new kernel = {rows['old'][i]['kernel_ms'] / max(rows['new'][i]['kernel_ms'], 1e-9):.2f}"
                         f"  wall = {rows['old'][i]['wall_ms'] / max(rows['new'][i]['wall_ms'], 1e-9):.2f}")
            lines.append(f"{shape:5s} round {i + 1}: " + "   ".join(parts) + ratio)
        for m in modes:
            ks = [r["kernel_ms"] for r in rows[m]]
            lines.append(f"{shape:5s} {m}: kernel median {statistics.median(ks):.3f} ms, spread between alternations "
                         f"{(max(ks) - min(ks)) / statistics.median(ks) * 100:.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
