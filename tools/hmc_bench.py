#!/usr/bin/env python3
"""Price the HMC step of MCMC.model_mh / gp_mh(chains=M, update='hmc', leapfrog=L) against the Langevin step and the random walk
of the same build, in the same process, on the same box, in the same run.

    python tools/hmc_bench.py [--parts maps gp] [--L 1 2 4 8] [--M 1024 65536] [--steps 400] [--burn 100]
                              [--kinds elliptic banana] [--dtypes float64 float32] [--delta-rw 0.7]
                              [--shapes N1 N2] [--modes gamma var] [--delta-gp 0.5 0.15] [--delta-gp-rw 0.5]

maps   the problems of tools/map_langevin_bench.py (elliptic, banana; delta = 1.4 and 0.5, the Langevin steps): the fused kernel
       (cesx_mh_hmc_run_map) and the step path (cesx_mh_hmc_begin, then per leapfrog cesx_map_jac and cesx_mh_hmc_leap /
       _accept) at every L, next to the fused and the step-path Langevin step and the fused random walk.  The cost model to
       compare with is L gradient evaluations and one test: ``fused_over_L_langevin`` is the fused HMC step over L times the
       fused Langevin step of the same row.
gp     the emulators of tools/gp_chain_bench.py (N1: 2 GPs, J_t = 50; N2: 9 GPs, J_t = 100) in the likelihood modes Gamma and
       diag(gvars): the HMC step path (per leapfrog cesx_gp_predict_grad and cesx_gp_hmc_leap / _accept) at every L and every
       ``--delta-gp``, next to the Langevin step at the same steps and the random walk at ``--delta-gp-rw``;
       ``over_L_langevin`` is the HMC step over L times the Langevin step at the same delta.
Every sampler runs ``summary=True, burn=...`` with ``noise='device'`` and ``start='mean'``; each figure is the second of two
calls on a fresh sampler (the first, 20 steps, pays the engine and the allocations).  No step is tuned: the accept rates are
printed next to the figures.
Prints one JSON line:
    maps, gp        rows per problem / M / dtype (mode): for every sampler ``*_us`` per step (wall time of the call over its steps,
                    host work included), ``accept_*``, ``ess_*`` (the smallest ``summary['ess']`` over the parameters) and
                    ``ess_per_s_*`` (over the wall time of the call)
    clock_ghz       the in-kernel clock class of the box (cesx_calibrate_mfma)
Nothing of this enters bench.py's value and nothing is asserted: the rows where HMC loses are part of the record.
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
from map_langevin_bench import DELTA, problem  # noqa: E402


def timed(mc, call, steps, burn):
    """The second of two calls on the fresh sampler ``mc``: (wall seconds, the row entries but the tag)."""
    import torch
    for n_mcmc, b in ((20, 0), (steps, burn)):
        mc.__dict__.pop("samples", None)
        mc.__dict__.pop("_mh_next_step", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(n_mcmc, b)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    ess = float(np.min(mc.summary["ess"]))
    _, ghz = mc._mh_eng.calibrate_mfma()
    mc._mh_eng.close()
    return ghz, dict(us=round(wall * 1e6 / steps, 2), accept=round(float(mc.accept), 4), ess=round(ess, 1),
                     ess_per_s=round(ess / wall, 1))


def main():
    from scipy import stats
    from ces_amd import calibrate, sample
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["maps", "gp"])
    ap.add_argument("--L", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--kinds", nargs="+", default=["elliptic", "banana"])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--delta-rw", type=float, default=0.7)
    ap.add_argument("--shapes", nargs="+", default=["N1", "N2"])
    ap.add_argument("--modes", nargs="+", default=["gamma", "var"])
    ap.add_argument("--delta-gp", type=float, nargs="+", default=[0.5, 0.15])
    ap.add_argument("--delta-gp-rw", type=float, default=0.5)
    args = ap.parse_args()
    out, ghz = dict(maps=[], gp=[]), 0.0

    def fresh(y, dtype):
        mc = sample.MCMC()
        mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", dtype
        return mc

    for kind in args.kinds if "maps" in args.parts else ():
        model, y, Gamma, mean, cov, ens = problem(kind)
        prior = stats.multivariate_normal(mean=mean, cov=cov)
        enka = calibrate.enka(2, 2, 130)
        enka.Ustar = ens
        for M in args.M:
            for dtype in args.dtypes:
                row = dict(kind=kind, M=M, dtype=dtype, steps=args.steps, burn=args.burn)
                runs = [("rw_fused", dict(update=None, fused=True, delta=args.delta_rw)),
                        ("langevin_fused", dict(update="langevin", fused=True, delta=DELTA[kind])),
                        ("langevin_step", dict(update="langevin", fused=False, delta=DELTA[kind]))]
                for L in args.L:
                    runs.append(("hmc%d_fused" % L, dict(update="hmc", leapfrog=L, fused=True, delta=DELTA[kind])))
                    runs.append(("hmc%d_step" % L, dict(update="hmc", leapfrog=L, fused=False, delta=DELTA[kind])))
                for tag, kw in runs:
                    mc = fresh(y, dtype)
                    ghz, res = timed(mc, lambda n, b: mc.model_mh(model, n, prior, enka, Gamma, chains=M, summary=True, burn=b, **kw),
                                     args.steps, args.burn)
                    row.update({"%s_%s" % (k, tag): v for k, v in res.items()})
                for L in args.L:
                    row["fused_over_L_langevin_%d" % L] = round(row["us_hmc%d_fused" % L] / (L * row["us_langevin_fused"]), 2)
                out["maps"].append(row)
                print("# %s" % json.dumps(row), file=sys.stderr, flush=True)

    for name in args.shapes if "gp" in args.parts else ():
        sh = SHAPES[name]
        p, n = sh["p"], sh["n"]
        enka = emulator(p, n, sh["Jt"], np.random.default_rng(0))
        y = enka.Gstar.mean(axis=1)
        prior = stats.multivariate_normal(mean=np.zeros(p), cov=4.0 * np.identity(p))
        for M in args.M:
            for mode in args.modes:
                like = dict(Gamma=0.05 * np.identity(n)) if mode == "gamma" else {}
                row = dict(shape=name, M=M, mode=mode, steps=args.steps, burn=args.burn)
                runs = [("rw", dict(update=None, delta=args.delta_gp_rw))]
                for d in args.delta_gp:
                    runs.append(("langevin_d%g" % d, dict(update="langevin", delta=d)))
                    runs += [("hmc%d_d%g" % (L, d), dict(update="hmc", leapfrog=L, delta=d)) for L in args.L]
                for tag, kw in runs:
                    mc = fresh(y, "float64")
                    ghz, res = timed(mc, lambda n_, b: mc.gp_mh(enka, n_, prior, chains=M, summary=True, burn=b, **kw, **like),
                                     args.steps, args.burn)
                    row.update({"%s_%s" % (k, tag): v for k, v in res.items()})
                for d in args.delta_gp:
                    for L in args.L:
                        row["over_L_langevin_%d_d%g" % (L, d)] = round(row["us_hmc%d_d%g" % (L, d)] / (L * row["us_langevin_d%g" % d]), 2)
                out["gp"].append(row)
                print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    out["clock_ghz"] = round(ghz, 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
