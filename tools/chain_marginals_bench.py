#!/usr/bin/env python3
"""Price ``marginals=`` (cesx_chain_hist_*: histograms of the kept states counted on the device): the stage's launches alone,
device events around ``chain_hist_add``, per draw.

    python tools/chain_marginals_bench.py [--steps 1000] [--reps 3 8]

Shapes (those of ``tools/chain_summary_bench.py --only kernels``, whose per-draw cost of ``chain_summary_add`` is the yardstick:
run it in the same session on the same box):
elliptic   p = 2, 65 536 chains, fp64, `steps` draws per add (a fused launch's trace)
lineal     p = 256, 65 536 chains, fp32, one draw per add (the step path)
Variants: the 1-D histograms alone (64 bins), and with 1, 8 and 64 pairs (20 x 20).  Draws: ``spread`` -- normal draws over the
range (6 standard deviations to either side) -- and ``one_bin`` -- every chain and draw the same value: every lane of every wave
adds to one counter, the worst contention.
``floor_us`` is the trace read once at ``--hbm-tbs`` TB/s (the 1-D kernel reads it once; the pairs' rows are read again).
Prints one JSON line; clock_ghz is the in-kernel clock class of the box (cesx_calibrate_mfma).  Nothing of this enters
bench.py's value.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIR_COUNTS = (0, 1, 8, 64)


def pairs_of(p, n):
    """n distinct pairs (i, j), i != j, of p rows; p = 2 has two, (0, 1) and (1, 0), and repeats them."""
    out, k = [], 0
    while len(out) < n:
        i = k % p
        j = (i + 1 + k // p) % p
        if i != j:
            out.append((i, j))
        k += 1
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def main():
    import torch
    from ces_amd import engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, nargs=2, default=[3, 8])
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the HBM rate the floor is taken at (a streaming copy sustains about 6.3 of the 8 TB/s)")
    args = ap.parse_args()
    out = {}
    for name, p, M, dtype, kept, reps in (("elliptic", 2, 65536, "float64", args.steps, args.reps[0]),
                                          ("lineal", 256, 65536, "float32", 1, args.reps[1])):
        eng = engine.Engine(p, p, M, dtype=dtype)
        e1 = np.stack([np.linspace(-6.0, 6.0, 65)] * p)
        e2 = np.stack([np.linspace(-6.0, 6.0, 21)] * p)
        nbytes = kept * p * M * eng.np_dtype.itemsize
        res = dict(p=p, chains=M, dtype=dtype, draws_per_add=kept, floor_us_per_draw=round(nbytes / (args.hbm_tbs * 1e6) / kept, 3))
        for draws in ("spread", "one_bin"):
            if draws == "spread":
                t = torch.randn((kept, p, M), dtype=eng.torch_dtype, device=eng.device)
            else:
                t = torch.full((kept, p, M), 0.3, dtype=eng.torch_dtype, device=eng.device)
            for n in PAIR_COUNTS:
                eng.chain_hist_begin(e1, e2, pairs_of(p, n))
                eng.chain_hist_add(t)                              # (the first add pays the module load)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(reps):
                    eng.chain_hist_add(t)
                b.record()
                torch.cuda.synchronize()
                res["%s/pairs%d_us_per_draw" % (draws, n)] = round(a.elapsed_time(b) * 1e3 / (reps * kept), 3)
                counts = eng.chain_hist_read()
                total = (reps + 1) * kept * M
                assert np.all(counts["hist1d"].sum(axis=1) + counts["below"] + counts["above"] == total)
                assert np.all(counts["hist2d"].sum(axis=(1, 2)) + counts["outside2d"] == total)
            del t
        out["kernels/%s" % name] = res
        out["clock_ghz"] = round(eng.calibrate_mfma()[1], 3)
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
