#!/usr/bin/env python3
"""Price the fused chain kernel of MCMC.gp_mh (cesx_gp_run: K Metropolis steps on the emulator per launch, one workgroup per
32 chains) against the step path (propose / gp_predict / gp_accept: three launches per step, four with the device noise of
an fp64 engine, and the copy of U where the trace keeps the step), in the same process and on the same engine.

    python tools/gp_chain_bench.py [--M 1 1024 65536] [--shapes N1 N2 E1] [--modes var gamma] [--strides 1 100]
                                   [--dtype float64] [--trace-bytes 1073741824]

Shapes (the reference's notebooks run p = 2, 2 to 10 GPs, J_t = 50 to 100 and 5 000 to 10 000 steps):
    N1   p = 2, 2 GPs, J_t = 50, 10 000 steps
    N2   p = 2, 9 GPs, J_t = 100, 5 000 steps
    E1   65 536 chains, p = 8, 32 GPs, J_t = 512 (tools/gp_bench.py), 5 steps, mode var, through the engine itself
N1 and N2 run ``gp_mh(chains=M)`` with Matern-3/2 ARD GPs and a Linear mean, a random walk, ``noise='device'``,
``start='mean'``, for every M, mode ('var': Gamma None; 'gamma': a diagonal Gamma) and ``trace_stride``.  A run whose kept
states would take more than --trace-bytes on the host runs fewer steps (the figure is per step); `steps` says how many ran.
Each figure is the second of two calls on one sampler (the first, 20 steps, pays the engine and the allocations).
Prints one JSON line:
    rows            per shape / M / mode / stride: steps, step_us and fused_us per Metropolis step (wall time of the
                    ``gp_mh`` call over its steps, host work included), ratio = step_us / fused_us, launches (fused),
                    accept_step and accept_fused (the same chains up to the few decisions among millions that sit within
                    rounding of their threshold)
    e1              step_ms and fused_ms per step at E1, ratio
    clock_ghz       the in-kernel clock class of the box (cesx_calibrate_mfma)
    fused_faster    the rows where fused_us < step_us, as a count of all rows
Nothing of this enters bench.py's value, and nothing is asserted about the ratios: the rows where fused is slower are what
keeps MCMC.GP_FUSED_DEFAULT at False.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"N1": dict(p=2, n=2, Jt=50, steps=10000), "N2": dict(p=2, n=9, Jt=100, steps=5000)}


class Enka(object):
    pass


def emulator(p, n, Jt, rng, lik=1e-4):
    from ces_amd import emulate as em
    U = rng.standard_normal((p, Jt))
    gps = []
    for i in range(n):
        y = np.sin(U[i % p]) + 0.1 * U.sum(0) + 0.1 * i
        m = em.GPR(U.T, y[:, None], em.Matern32(input_dim=p, ARD=True, lengthscales=1.5 + rng.random(p)),
                   mean_function=em.Linear(0.1 * rng.standard_normal((p, 1)), [0.0]))
        m.likelihood.variance = lik
        gps.append(m)
    enka = Enka()
    enka.p, enka.n_obs, enka.Ustar, enka.gpmodels = p, n, U, gps
    enka.Gstar = np.array([np.sin(U[i % p]) + 0.1 * U.sum(0) + 0.1 * i for i in range(n)])
    return enka


def notebook_rows(args, out):
    import torch
    from scipy import stats
    from ces_amd import sample
    ghz = 0.0
    for name in [s for s in args.shapes if s in SHAPES]:
        sh = SHAPES[name]
        p, n = sh["p"], sh["n"]
        enka = emulator(p, n, sh["Jt"], np.random.default_rng(0))
        y = enka.Gstar.mean(axis=1)
        prior = stats.multivariate_normal(mean=np.zeros(p), cov=4.0 * np.identity(p))
        for M in args.M:
            for mode in args.modes:
                kw = dict(Gamma=0.05 * np.identity(n)) if mode == "gamma" else {}
                for stride in args.strides:
                    steps = min(sh["steps"], max(stride, args.trace_bytes // (M * p * 8) * stride))
                    mc = sample.MCMC()
                    mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype, mc.trace_stride = True, y, "device", args.dtype, stride
                    us, acc, launches = {}, {}, 0
                    for fused in (False, True):
                        for n_mcmc in (20, steps):
                            mc.__dict__.pop("samples", None)
                            mc.__dict__.pop("_mh_next_step", None)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            mc.gp_mh(enka, n_mcmc, prior, delta=0.5, chains=M, fused=fused, **kw)
                            torch.cuda.synchronize()
                            us[fused] = (time.perf_counter() - t0) * 1e6 / n_mcmc
                        acc[fused] = float(mc.accept)
                        launches = mc.fused_launches
                    _, ghz = mc._mh_eng.calibrate_mfma()
                    mc._mh_eng.close()
                    out["rows"].append(dict(shape=name, M=M, mode=mode, stride=stride, steps=steps, step_us=round(us[False], 2),
                                            fused_us=round(us[True], 3), ratio=round(us[False] / us[True], 2),
                                            launches=launches, accept_step=round(acc[False], 4),
                                            accept_fused=round(acc[True], 4)))
                    print("# %s" % json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    return ghz


def e1(args, out):
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    p, n, M, Jt, steps = 8, 32, 65536, 512, 5
    rng = np.random.default_rng(0)
    enka = emulator(p, n, Jt, rng)
    eng = engine.Engine(p, n, M, dtype=args.dtype)
    eng.set_problem(np.zeros(n), np.eye(n), np.zeros(p), np.eye(p), np.zeros(p))
    eng.mh_set_proposal(None, 0.05 * np.eye(p))
    eng.gp_set(em.device_image(enka, enka.gpmodels))
    X0 = eng.to_device(0.5 * rng.standard_normal((p, M)), p)
    P = eng.empty(p)
    mean = torch.empty((n, M), dtype=torch.float64, device=eng.device)
    var = torch.empty_like(mean)
    ms = {}
    for fused in (False, True):
        X = X0.clone()
        eng.gp_predict(X, out=(mean, var))
        eng.gp_start("var", X, mean, var)
        for rep in range(2):                              # (the second is timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if fused:
                eng.gp_run("var", rep * steps, steps, X)
            else:
                for s in range(rep * steps, (rep + 1) * steps):
                    eng.mh_propose(s, X, out=P)
                    eng.gp_predict(P, out=(mean, var))
                    eng.gp_accept("var", s, X, P, mean, var)
            torch.cuda.synchronize()
            ms[fused] = (time.perf_counter() - t0) * 1e3 / steps
    _, ghz = eng.calibrate_mfma()
    eng.close()
    out["e1"] = dict(chains=M, p=p, n_gp=n, J_t=Jt, steps=steps, step_ms=round(ms[False], 3), fused_ms=round(ms[True], 3),
                     ratio=round(ms[False] / ms[True], 2))
    return ghz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[1, 1024, 65536])
    ap.add_argument("--shapes", nargs="+", default=["N1", "N2", "E1"])
    ap.add_argument("--modes", nargs="+", default=["var", "gamma"])
    ap.add_argument("--strides", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--trace-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    out = dict(rows=[])
    ghz = notebook_rows(args, out)
    if "E1" in args.shapes:
        ghz = e1(args, out)
    out["clock_ghz"] = round(ghz, 3)
    out["fused_faster"] = "%d of %d" % (sum(r["fused_us"] < r["step_us"] for r in out["rows"]), len(out["rows"]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
