#!/usr/bin/env python3
"""Price the adaptation step of MCMC.model_mh / gp_mh(chains=M, adapt=) and record what it finds, in one process on one box.

    python tools/adapt_bench.py [--parts cost found] [--M 1024 65536] [--L 1 4] [--steps 400] [--adapt 100]

cost   wall time per step of the step path on an ARMED engine (cesx_mh_adapt_set: the ADAPT kernels of kernels_hmc.hip and
       ad_update_kernel behind every accept) against the same steps on the same engine unarmed -- the leapfrog step path as it
       was before adaptation existed; the difference is one small launch and a uniform load per kernel.  Shapes: the elliptic
       map (cesx_map_jac per leapfrog) and the emulator N1 of tools/gp_chain_bench.py (2 GPs, J_t = 50, Sigma = Gamma;
       cesx_gp_predict_grad per leapfrog).  fp64, device noise, ``--steps`` steps after 20 warm-up steps, nothing copied to the
       host in between.
found  the emulator N2 (9 GPs, J_t = 100) with Sigma = diag(gvars) at ``delta=0.5``, where update='langevin' accepts nothing
       (tools/gp_langevin_bench.py): ``adapt=--adapt`` of ``--adapt + --steps`` steps with ``summary=True, burn=--adapt`` --
       the multiplier found, the acceptance at the frozen step and ``summary['ess']`` per second of the whole call, adaptation
       included -- next to the hand-tuned ``delta=0.15`` and the unadapted ``delta=0.5`` run of ``--steps`` steps.
Prints one JSON line: ``cost`` and ``found`` rows and ``clock_ghz`` (cesx_calibrate_mfma).  Nothing is asserted and nothing of
this enters bench.py's value.
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

WARM = 20


def time_steps(eng, one_step, steps, target):
    """(unarmed us per step, armed us per step) of ``one_step(k)`` on ``eng``, each after WARM steps of its own."""
    import torch
    res = []
    for armed in (False, True):
        if armed:
            eng.mh_adapt_set(WARM + steps, target)
        for k in range(WARM):
            one_step(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(WARM, WARM + steps):
            one_step(k)
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) * 1e6 / steps)
    return res


def cost_rows(args):
    import torch
    from ces_amd import emulate, engine, sample
    rows, ghz = [], 0.0
    for shape in ("elliptic", "N1"):
        for M in args.M:
            for L in args.L:
                target = sample.ADAPT_TARGETS["langevin" if L == 1 else "hmc"]
                if shape == "elliptic":
                    model, y, Gamma, mean, cov, ens = problem("elliptic")
                    p, n = 2, 2
                    S = DELTA["elliptic"] * np.linalg.cholesky(np.cov(ens))
                    U0 = np.repeat(ens.mean(axis=1)[:, None], M, axis=1)
                else:
                    sh = SHAPES[shape]
                    p, n = sh["p"], sh["n"]
                    enka = emulator(p, n, sh["Jt"], np.random.default_rng(0))
                    y, Gamma, mean, cov = enka.Gstar.mean(axis=1), 0.05 * np.identity(n), np.zeros(p), 4.0 * np.identity(p)
                    S = 0.15 * np.linalg.cholesky(np.cov(enka.Ustar))
                    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
                eng = engine.Engine(p, n, M, dtype="float64")
                eng.set_problem(y, Gamma, mean, cov, mean)
                eng.mh_set_proposal("hmc", S)
                U, Q = eng.to_device(U0, p, "U0").clone(), eng.empty(p)
                if shape == "elliptic":
                    model.ensure_installed(eng)
                    out = model.jacobian_device(eng, U)
                    eng.mh_langevin_start(U, *out)

                    def one_step(k):
                        eng.mh_hmc_begin(k, U, out=Q)
                        for _ in range(L - 1):
                            model.jacobian_device(eng, Q, out=out)
                            eng.mh_hmc_leap(Q, *out)
                        model.jacobian_device(eng, Q, out=out)
                        eng.mh_hmc_accept(k, U, Q, *out)
                else:
                    eng.gp_set(emulate.device_image(enka, enka.gpmodels))
                    out = (torch.empty((n, M), dtype=torch.float64, device=eng.device), None,
                           torch.empty((n, p, M), dtype=torch.float64, device=eng.device), None)
                    eng.gp_predict_grad(U, nugget=True, var=False, out=out)
                    eng.gp_langevin_start("gamma", U, *out)

                    def one_step(k):
                        eng.mh_hmc_begin(k, U, out=Q)
                        for _ in range(L - 1):
                            eng.gp_predict_grad(Q, nugget=True, var=False, out=out)
                            eng.gp_hmc_leap("gamma", Q, *out)
                        eng.gp_predict_grad(Q, nugget=True, var=False, out=out)
                        eng.gp_hmc_accept("gamma", k, U, Q, *out)
                plain, armed = time_steps(eng, one_step, args.steps, target)
                found = eng.mh_adapt_read()
                _, ghz = eng.calibrate_mfma()
                eng.close()
                row = dict(shape=shape, M=M, L=L, steps=args.steps, us_step=round(plain, 2), us_adapt_step=round(armed, 2),
                           us_more=round(armed - plain, 2), ratio=round(armed / plain, 3), multiplier=round(found["multiplier"], 4))
                rows.append(row)
                print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    return rows, ghz


def found_rows(args):
    import torch
    from scipy import stats
    from ces_amd import sample
    sh = SHAPES["N2"]
    p, n = sh["p"], sh["n"]
    enka = emulator(p, n, sh["Jt"], np.random.default_rng(0))
    y = enka.Gstar.mean(axis=1)
    prior = stats.multivariate_normal(mean=np.zeros(p), cov=4.0 * np.identity(p))
    rows = []
    for M in args.M:
        for tag, delta, adapt in (("adapt", 0.5, args.adapt), ("tuned", 0.15, 0), ("untuned", 0.5, 0)):
            for warm in (True, False):                    # the second of two calls on a fresh sampler, as tools/hmc_bench.py times
                mc = sample.MCMC()
                mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", "float64"
                n_mcmc = 24 if warm else adapt + args.steps
                A = (8 if warm else adapt) if adapt else 0
                kw = dict(adapt=A, burn=A) if A else dict(burn=0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mc.gp_mh(enka, n_mcmc, prior, delta=delta, chains=M, update="langevin", summary=True, **kw)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                if warm:
                    mc._mh_eng.close()
            ess = float(np.min(mc.summary["ess"]))      # (NaN where nothing was accepted: no variance between the half-chains)
            row = dict(shape="N2", mode="var", M=M, run=tag, delta=delta, steps=n_mcmc, adapt=A, accept=round(float(mc.accept), 4),
                       ess=round(ess, 1) if np.isfinite(ess) else None, wall_s=round(wall, 4),
                       ess_per_s=round(ess / wall, 1) if np.isfinite(ess) else None)
            if A:
                row.update(multiplier=round(mc.adapt["multiplier"], 5), delta_found=round(mc.adapt["delta"], 5))
            mc._mh_eng.close()
            rows.append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["cost", "found"])
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--L", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--adapt", type=int, default=100)
    args = ap.parse_args()
    out, ghz = dict(cost=[], found=[]), 0.0
    if "cost" in args.parts:
        out["cost"], ghz = cost_rows(args)
    if "found" in args.parts:
        out["found"] = found_rows(args)
    out["clock_ghz"] = round(ghz, 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
