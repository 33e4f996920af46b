#!/usr/bin/env python3
"""Price the Langevin step of MCMC.gp_mh(chains=M, update='langevin') (cesx_gp_predict_grad + cesx_gp_langevin_*: the GP rows
with their gradients, then propose and accept, per step) against the random-walk step path (cesx_mh_propose / cesx_gp_predict /
cesx_gp_accept) in the same process, on the same box, in the same run.

    python tools/gp_langevin_bench.py [--M 1024 65536] [--shapes N1 N2] [--modes gamma var] [--steps 400] [--burn 100]
                                      [--delta-rw 0.5] [--delta-langevin 0.5] [--dtype float64]

Shapes (tools/gp_chain_bench.py's: the reference's notebooks run p = 2, 2 to 10 GPs, J_t = 50 to 100):
    N1   p = 2, 2 GPs, J_t = 50
    N2   p = 2, 9 GPs, J_t = 100
Both samplers run ``gp_mh(chains=M, summary=True, burn=...)`` with Matern-3/2 ARD GPs and a Linear mean, ``noise='device'``,
``start='mean'``; each figure is the second of two calls on a fresh sampler (the first, 20 steps, pays the engine and the
allocations).  Neither step size is tuned: the accept rates are printed next to the figures.
Prints one JSON line:
    rows            per shape / M / mode: steps, rw_us and langevin_us per Metropolis step (wall time of the ``gp_mh`` call over
                    its steps, host work included), ratio = langevin_us / rw_us, accept_rw and accept_langevin, ess_rw and
                    ess_langevin (the smallest ``summary['ess']`` over the parameters: the split between-half-chain estimate, capped at
                    the number of draws), ess_per_s_rw and ess_per_s_langevin (ess over the wall time of the call), and
                    rhat_rw / rhat_langevin (the largest)
    clock_ghz       the in-kernel clock class of the box (cesx_calibrate_mfma)
    langevin_wins   the rows where ess_per_s_langevin > ess_per_s_rw, as a count of all rows
Nothing of this enters bench.py's value and nothing is asserted: the rows where Langevin loses are part of the record.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gp_chain_bench import SHAPES, emulator  # noqa: E402


def main():
    import torch
    from scipy import stats
    from ces_amd import sample
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--shapes", nargs="+", default=["N1", "N2"])
    ap.add_argument("--modes", nargs="+", default=["gamma", "var"])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--delta-rw", type=float, default=0.5)
    ap.add_argument("--delta-langevin", type=float, default=0.5)
    ap.add_argument("--dtype", default="float64")
    args = ap.parse_args()
    out, ghz = dict(rows=[]), 0.0
    for name in args.shapes:
        sh = SHAPES[name]
        p, n = sh["p"], sh["n"]
        enka = emulator(p, n, sh["Jt"], np.random.default_rng(0))
        y = enka.Gstar.mean(axis=1)
        prior = stats.multivariate_normal(mean=np.zeros(p), cov=4.0 * np.identity(p))
        for M in args.M:
            for mode in args.modes:
                kw = dict(Gamma=0.05 * np.identity(n)) if mode == "gamma" else {}
                row = dict(shape=name, M=M, mode=mode, steps=args.steps, burn=args.burn)
                for tag, update, delta in (("rw", None, args.delta_rw), ("langevin", "langevin", args.delta_langevin)):
                    mc = sample.MCMC()
                    mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", args.dtype
                    for n_mcmc, burn in ((20, 0), (args.steps, args.burn)):
                        mc.__dict__.pop("samples", None)
                        mc.__dict__.pop("_mh_next_step", None)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        mc.gp_mh(enka, n_mcmc, prior, delta=delta, chains=M, update=update, summary=True, burn=burn, **kw)
                        torch.cuda.synchronize()
                        wall = time.perf_counter() - t0
                    ess = float(np.min(mc.summary["ess"]))
                    row.update({"%s_us" % tag: round(wall * 1e6 / args.steps, 2), "accept_%s" % tag: round(float(mc.accept), 4),
                                "ess_%s" % tag: round(ess, 1), "ess_per_s_%s" % tag: round(ess / wall, 1),
                                "rhat_%s" % tag: round(float(np.max(mc.summary["rhat"])), 4)})
                    _, ghz = mc._mh_eng.calibrate_mfma()
                    mc._mh_eng.close()
                row["ratio"] = round(row["langevin_us"] / row["rw_us"], 2)
                out["rows"].append(row)
                print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    out["clock_ghz"] = round(ghz, 3)
    out["langevin_wins"] = "%d of %d" % (sum(r["ess_per_s_langevin"] > r["ess_per_s_rw"] for r in out["rows"]), len(out["rows"]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
