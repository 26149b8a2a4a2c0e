#!/usr/bin/env python3
"""Tiled size sweep (k > sweep_max_assets()) against what a caller does at the parent commit, timed with the library's own HIP
events.

    python tools/time_size_sweep_tiled.py --parent DIR [--rounds 3] [--out FILE]

DIR is a checkout of the parent commit with its library built (make -C DIR/incorporating_different_sources_amd/csrc).
Every measurement runs in a fresh child process under a time limit of its own; a child that fails ends the measurement.
"old" imports the package of DIR and runs ONE batch per size over the prefix columns, every window's arrays repeated once
per prior (P x W windows per batch) - four packs, uploads and batches for four sizes; "new" imports this tree, uploads the W
windows once at the largest size and runs one tiled size sweep.  Old and new alternate `--rounds` times; the chain stops at
the first child that fails.  Shapes (sizes k/4 .. k in four steps, except grid's 200 / 300 / 400 / 500):

    grid     k = 500, 249 daily rows, 5 intraday days, index layout as batch.pack_windows emits it, W = 256, conjugate, P = 4
    gridj    the same, Jeffreys (P = 1)
    c3       k = 500, W = 4,096, contiguous (the intraday panel repeats after 32 days), conjugate, P = 1
    k1000    k = 1000, sizes 250 / 500 / 750 / 1000, otherwise as grid, W = 64, conjugate, P = 4

kernel_ms is tp_last_timing's kernel span (old: summed over the sizes), median of `--reps` repetitions after one warm-up;
wall_ms is the host time of one whole repetition, batch creation, uploads and downloads included.
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

# k, N, W, P, index layout, conjugate, sizes, hf_period
SHAPES = {"grid": (500, 250, 256, 4, True, True, [200, 300, 400, 500], 0),
          "gridj": (500, 250, 256, 1, True, False, [200, 300, 400, 500], 0),
          "c3": (500, 250, 4096, 1, False, True, [200, 300, 400, 500], 32),
          "k1000": (1000, 250, 64, 4, True, True, [250, 500, 750, 1000], 0)}
HF_DAYS = 5


def inputs(np, synthetic, k, N, W, P, index, SIZES, hf_period):
    inp = synthetic.make_kernel_inputs(k, N, W, seed=20250915, hf_days=HF_DAYS, hf_period=hf_period)
    rng = np.random.default_rng(20250915)
    n_r = inp["n_r"]
    kw = dict(panel=inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"])
    if index:
        extra = 14
        kw["panel"] = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], extra))], axis=1)
        kw["hf_panel"] = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], extra))], axis=1)
        del kw["start"]
        kw.update(row_idx=(inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32),
                  n_rows=np.full(W, n_r, dtype=np.int32),
                  col_idx=np.stack([rng.permutation(k + extra)[:k] for _ in range(W)]).astype(np.int32),
                  rf_adj=rng.normal(0, 1e-4, size=(W, n_r)))
    scal = np.array([1, 5])[(np.arange(P) // 2) % 2]
    n0 = N * scal[None, :] * rng.uniform(1.0, 1.6, size=(W, P))
    caps = -np.sort(-rng.lognormal(0.0, 1.0, size=(W, k)), axis=1)
    w0 = np.zeros((W, P, len(SIZES), k))
    for s, ks in enumerate(SIZES):
        vw = caps[:, :ks] / caps[:, :ks].sum(axis=1, keepdims=True)
        w0[:, :, s, :ks] = np.where((np.arange(P) % 2 == 1)[None, :, None], vw[:, None, :], 1.0 / ks)
    return kw, np.ascontiguousarray(n0), w0, n_r, inp["m"]


def child(mode, shape, reps):
    import numpy as np
    from incorporating_different_sources_amd import _native, synthetic
    k, N, W, P, index, conj, SIZES, hf_period = SHAPES[shape]
    kw, n0, w0, n_r, m = inputs(np, synthetic, k, N, W, P, index, SIZES, hf_period)
    if not conj:
        kw = {key: val for key, val in kw.items() if not key.startswith("hf_")}
    strategy = "conjugate" if conj else "jeffreys"
    dev = _native.Device(0)
    res = dict(mode=mode, shape=shape, lib=_native.LIB_PATH)
    per_window = ("start", "row_idx", "n_rows", "col_idx", "rf_adj", "hf_start")

    def once():
        t0 = time.perf_counter()
        ms = 0.0
        if mode == "old":
            for s, ks in enumerate(SIZES):
                sub = dict(kw)
                if index:
                    sub["col_idx"] = np.ascontiguousarray(kw["col_idx"][:, :ks])
                else:
                    sub["panel"] = np.ascontiguousarray(kw["panel"][:, :ks])
                    if conj:
                        sub["hf_panel"] = np.ascontiguousarray(kw["hf_panel"][:, :ks])
                big = {key: (np.concatenate([val] * P, axis=0) if key in per_window else val) for key, val in sub.items()}
                b = _native.Batch(dev, strategy, ks, N, n_r, 5.0, P * W, m if conj else 0)
                if conj:
                    big.update(w0=np.ascontiguousarray(w0[:, :, s, :ks].transpose(1, 0, 2)).reshape(P * W, ks),
                               n0=np.ascontiguousarray(n0.T).reshape(P * W))
                b.upload(**big)
                b.run().download(want_aux=False)
                ms += dev.last_timing()["kernel_ms"]
                b.close()
        else:
            b = _native.Batch(dev, strategy, k, N, n_r, 5.0, W, m if conj else 0)
            if conj:
                b.upload(w0=w0[:, 0, -1], n0=n0[:, 0], **kw)
                b.size_sweep_tiled(SIZES, n0, w0, want_aux=False)
            else:
                b.upload(**kw)
                b.size_sweep_tiled(SIZES, want_aux=False)
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
    ap.add_argument("--shapes", default="grid,gridj,c3,k1000")
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
                print(f"  ({shape} {mode}: kernel {rows[mode][-1]['kernel_ms']:.3f} ms)", flush=True)
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
