#!/usr/bin/env python3
"""Large-k (tiled) prior sweep against the replicated batch of the parent commit, timed with the library's own HIP events.

    python tools/time_prior_sweep_tiled.py --parent DIR [--rounds 3] [--out FILE]

DIR is a checkout of the parent commit with its library built (make -C DIR/incorporating_different_sources_amd/csrc).
Every measurement runs in a fresh child process: "old" imports the package of DIR and runs what
calculate_weights_for_specs does there - every window's index arrays repeated once per prior, ONE batch of P x W windows -
"new" imports this tree, uploads the W windows once and runs one tiled prior sweep (Batch.prior_sweep_tiled).  Old and new alternate `--rounds` times.
Shapes:

    k500i16  k = 500, 249 daily + 5 x 78 - 1 intraday rows, index layout as batch.pack_windows emits it, W = 256, P = 16
    k500i4   the same with P = 4
    c3       k = 500, W = 4,096, contiguous (the shape of BASELINE configs[2]), P = 16: the parent's replicas get the shared
             block sums there, the sweep does not
    k191i16  k = 191, 249 + 77 rows, index layout, W = 256, P = 16

kernel_ms is tp_last_timing's kernel span, median of `--reps` repetitions after one warm-up; wall_ms is the host time of one
whole repetition, batch creation, upload and download included.
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

# (k, N, W, P, index layout, intraday days per window)
SHAPES = {"k500i16": (500, 250, 256, 16, True, 5), "k500i4": (500, 250, 256, 4, True, 5), "c3": (500, 250, 4096, 16, False, 5),
          "k191i16": (191, 250, 256, 16, True, 1)}


def inputs(np, synthetic, k, N, W, P, index, hf_days):
    inp = synthetic.make_kernel_inputs(k, N, W, seed=20250901, hf_days=hf_days, hf_period=256)
    rng = np.random.default_rng(20250901)
    n_r = inp["n_r"]
    kw = dict(panel=inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"])
    if index:
        extra = 14
        kw["panel"] = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], extra))], axis=1)
        kw["hf_panel"] = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], extra))], axis=1)
        del kw["start"]
        kw.update(row_idx=(inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32),
                  n_rows=np.full(W, n_r, dtype=np.int32),
                  col_idx=np.stack([np.sort(rng.permutation(k + extra)[:k]) for _ in range(W)]).astype(np.int32),
                  rf_adj=rng.normal(0, 1e-4, size=(W, n_r)))
    scal = np.array([0.001, 1, 5, 20])[(np.arange(P) // 2) % 4]
    n0 = N * scal[None, :] * rng.uniform(1.0, 1.6, size=(W, P))
    caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
    vw = caps / caps.sum(axis=1, keepdims=True)
    w0 = np.where((np.arange(P) % 2 == 1)[None, :, None], vw[:, None, :], 1.0 / k)
    return kw, np.ascontiguousarray(n0), np.ascontiguousarray(w0), n_r, inp["m"]


def child(mode, shape, reps):
    import numpy as np
    from incorporating_different_sources_amd import _native, synthetic
    k, N, W, P, index, hf_days = SHAPES[shape]
    kw, n0, w0, n_r, m = inputs(np, synthetic, k, N, W, P, index, hf_days)
    dev = _native.Device(0)
    res = dict(mode=mode, shape=shape, lib=_native.LIB_PATH)
    per_window = ("start", "row_idx", "n_rows", "col_idx", "rf_adj", "hf_start")

    def once():
        t0 = time.perf_counter()
        if mode == "old":
            big = {key: (np.concatenate([val] * P, axis=0) if key in per_window else val) for key, val in kw.items()}
            b = _native.Batch(dev, "conjugate", k, N, n_r, 5.0, P * W, m)
            b.upload(w0=np.ascontiguousarray(w0.transpose(1, 0, 2)).reshape(P * W, k),
                     n0=np.ascontiguousarray(n0.T).reshape(P * W), **big)
            b.run().download(want_aux=False)
        else:
            b = _native.Batch(dev, "conjugate", k, N, n_r, 5.0, W, m)
            b.upload(w0=w0[:, 0], n0=n0[:, 0], **kw)
            b.prior_sweep_tiled(n0, w0, want_aux=False)
        ms = dev.last_timing()["kernel_ms"]
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
    ap.add_argument("--shapes", default="k500i16,k500i4,c3,k191i16")
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
                ratio = (f"   old/new kernel = {rows['old'][i]['kernel_ms'] / max(rows['new'][i]['kernel_ms'], 1e-9):.2f}"
                         f"  wall = {rows['old'][i]['wall_ms'] / max(rows['new'][i]['wall_ms'], 1e-9):.2f}")
            lines.append(f"{shape:7s} round {i + 1}: " + "   ".join(parts) + ratio)
        for m in modes:
            ks = [r["kernel_ms"] for r in rows[m]]
            lines.append(f"{shape:7s} {m}: kernel median {statistics.median(ks):.3f} ms, spread between alternations "
                         f"{(max(ks) - min(ks)) / statistics.median(ks) * 100:.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
