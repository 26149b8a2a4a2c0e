"""Cost of keeping the posterior matrices (Batch.keep_posterior): step time with the option off and on (all windows), in one
process, alternating, on configs[1] (k = 100, contiguous and index layout), k = 191, k = 500 and k = 1000.  Prints one line
per point: median step times, the bytes the kept matrices add, the added time and the write rate it implies (bytes /
added time), and the bound bytes / 6.3 TB/s.  Needs the GPU.
    python tools/time_posterior_output.py [--steps 10] [--json out.json] [--only NAME]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from incorporating_different_sources_amd import _native, synthetic  # noqa: E402

HBM_BPS = 6.3e12


def points():
    c1 = synthetic.config_shapes(2)           # BASELINE configs[1]: k = 100, N = 250, 10,000 windows
    yield "configs[1] contiguous", c1["k"], c1["N"], c1["W"], c1["hf_days"], False
    yield "configs[1] index", c1["k"], c1["N"], c1["W"], c1["hf_days"], True
    yield "k=191", 191, 400, 8192, 3, False
    yield "k=500", 500, 250, 8192, 1, False
    yield "k=1000", 1000, 500, 4096, 1, False


def step_ms(dev, b, steps):
    b.run()
    dev.synchronize()
    dev.region_begin()
    for _ in range(steps):
        b.run()
    dev.region_end()
    return float(np.median(dev.region_steps()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="run the points whose name starts with this (e.g. 'configs[1] contiguous')")
    args = ap.parse_args()
    dev = _native.Device(0)
    rows = []
    for name, k, N, W, hf_days, index in points():
        if args.only and not name.startswith(args.only):
            continue
        inp = synthetic.make_kernel_inputs(k, N, W, seed=20240100 + k, hf_days=hf_days, hf_period=64)
        b = dev.batch("conjugate", k, N, inp["n_r"], 5.0, W, inp["m"])
        kw = dict(start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
        if index:
            kw.pop("start")
            kw.update(row_idx=(inp["start"][:, None] + np.arange(inp["n_r"])[None, :]).astype(np.int32),
                      col_idx=np.tile(np.arange(k, dtype=np.int32), (W, 1)))
        b.upload(inp["panel"], **kw)
        off, on = [], []
        for _ in range(3):                       # alternate: off, on, off, on, ...
            b.keep_posterior(0, 0)
            off.append(step_ms(dev, b, args.steps))
            b.keep_posterior()
            on.append(step_ms(dev, b, args.steps))
        b.close()
        t_off, t_on = float(np.median(off)), float(np.median(on))
        nbytes = 8.0 * W * k * k
        added = t_on - t_off
        row = dict(point=name, k=k, windows=W, step_ms_off=t_off, step_ms_on=t_on, added_ms=added, bytes_written=nbytes,
                   write_rate_tbs=(nbytes / (added * 1e-3) / 1e12) if added > 0 else None,
                   bound_ms_at_6_3_tbs=nbytes / HBM_BPS * 1e3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    dev.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
