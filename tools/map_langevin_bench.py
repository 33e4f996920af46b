#!/usr/bin/env python3
"""Price the Langevin step of MCMC.model_mh(chains=M, update='langevin') on the closed-form maps: the fused kernel
(cesx_mh_langevin_run_map: up to 4 096 steps per launch, the chain and its g in one lane's registers) against the step path
(cesx_mh_langevin_propose / cesx_map_jac / cesx_mh_langevin_accept per step) and against the fused random walk
(cesx_mh_run_map) of the same build, in the same process, on the same box, in the same run.

    python tools/map_langevin_bench.py [--kinds elliptic banana] [--M 1024 65536] [--dtypes float64 float32]
                                       [--steps 400] [--burn 100] [--delta-rw 0.7]

The problems are those of tests/map_cases.py (elliptic.ipynb's data with Gamma = 0.1^2 I, the banana with its dense Gamma; a
dense prior covariance), the Langevin steps delta = 1.4 (elliptic) and 0.5 (banana) with the scales of a 130-particle ensemble
near the posterior's bulk.  Every sampler runs ``model_mh(chains=M, summary=True, burn=...)`` with ``noise='device'`` and
``start='mean'``; each figure is the second of two calls on a fresh sampler (the first, 20 steps, pays the engine and the
allocations).
Prints one JSON line:
    rows            per kind / M / dtype: steps; fused_us, step_us and rw_fused_us per step (wall time of the ``model_mh`` call
                    over its steps, host work included); accept_* and ess_* (the smallest ``summary['ess']`` over the
                    parameters) and ess_per_s_* of the three samplers
    clock_ghz       the in-kernel clock class of the box (cesx_calibrate_mfma)
    fused_faster    per M, whether fused_us < step_us on the elliptic problem in fp64: what ``MCMC.LANGEVIN_FUSED_DEFAULT``
                    follows when both sizes agree (the step path otherwise)
Nothing of this enters bench.py's value and nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DELTA = {"elliptic": 1.4, "banana": 0.5}


def problem(kind):
    """(model, y, Gamma, prior mean, prior cov, start ensemble (2, 130))."""
    from ces_amd import utils
    rng = np.random.default_rng(4)
    if kind == "elliptic":
        return (utils.elliptic(), np.array([27.45194112300398, 79.70194112300398]), 0.1 ** 2 * np.identity(2),
                np.array([0.0, 100.0]), np.array([[4.0, 1.5], [1.5, 30.0]]),
                np.vstack([-2.65 + 0.05 * rng.standard_normal(130), 104.5 + 0.05 * rng.standard_normal(130)]))
    model = utils.banana()
    return (model, np.array([0.3, -0.4]), model.Gamma, np.array([0.2, -0.1]), np.array([[2.0, 0.6], [0.6, 3.0]]),
            np.vstack([0.3 + 0.4 * rng.standard_normal(130), 0.2 + 0.6 * rng.standard_normal(130)]))


def main():
    import torch
    from scipy import stats
    from ces_amd import calibrate, sample
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", nargs="+", default=["elliptic", "banana"])
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--delta-rw", type=float, default=0.7)
    args = ap.parse_args()
    out, ghz = dict(rows=[]), 0.0
    for kind in args.kinds:
        model, y, Gamma, mean, cov, ens = problem(kind)
        prior = stats.multivariate_normal(mean=mean, cov=cov)
        enka = calibrate.enka(2, 2, 130)
        enka.Ustar = ens
        for M in args.M:
            for dtype in args.dtypes:
                row = dict(kind=kind, M=M, dtype=dtype, steps=args.steps, burn=args.burn)
                for tag, update, fused, delta in (("fused", "langevin", True, DELTA[kind]), ("step", "langevin", False, DELTA[kind]),
                                                  ("rw_fused", None, True, args.delta_rw)):
                    mc = sample.MCMC()
                    mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", dtype
                    for n_mcmc, burn in ((20, 0), (args.steps, args.burn)):
                        mc.__dict__.pop("samples", None)
                        mc.__dict__.pop("_mh_next_step", None)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        mc.model_mh(model, n_mcmc, prior, enka, Gamma, delta=delta, chains=M, update=update, fused=fused,
                                    summary=True, burn=burn)
                        torch.cuda.synchronize()
                        wall = time.perf_counter() - t0
                    ess = float(np.min(mc.summary["ess"]))
                    row.update({"%s_us" % tag: round(wall * 1e6 / args.steps, 2), "accept_%s" % tag: round(float(mc.accept), 4),
                                "ess_%s" % tag: round(ess, 1), "ess_per_s_%s" % tag: round(ess / wall, 1)})
                    _, ghz = mc._mh_eng.calibrate_mfma()
                    mc._mh_eng.close()
                out["rows"].append(row)
                print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    out["clock_ghz"] = round(ghz, 3)
    out["fused_faster"] = {str(r["M"]): bool(r["fused_us"] < r["step_us"]) for r in out["rows"]
                           if r["kind"] == "elliptic" and r["dtype"] == "float64"}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
