#!/usr/bin/env python3
"""Price the leapfrog step of MCMC.model_mh(chains=M, update='hmc') on the linear map at the benchmark's shape
(p = n_obs = 256) against the Langevin and the random-walk step of the same build, in the same process, on the same box, in
the same run (tools/lineal_langevin_bench.py's problem, scalings and form).

    python tools/lineal_hmc_bench.py [--p 256] [--M 1024 65536] [--dtypes float32 float64] [--L 1 2 4 8] [--reps 50]
                                     [--ess-M 1024] [--steps 400] [--burn 100] [--starts mean ensemble] [--adapt 100]

The problem is Gaussian: A = randn / sqrt(p), Gamma = 0.1^2 I, Sigma = I, mu = 0, a 1 024-particle ensemble of exact posterior
draws for the scales.  The steps are the textbook scalings and are not tuned: random walk delta = 2.38 / sqrt(p), Langevin and
leapfrog delta = 1.65 p^(-1/6).
Prints one JSON line:
    rows    per M / dtype, in microseconds of DEVICE time per step (hip events on the stream; one event pair around ``reps``
            whole steps, after 5 warm-up steps of the same shape):
              lv_us, lv_us_again     the Langevin step (cesx_mh_langevin_lineal_*), measured before and after the leapfrog runs:
                                     their difference is the run-to-run spread of this process
              pieces = {begin, forward, leap, accept}    event pairs around each entry point of an L = 2 step (the markers add
                                     their own gaps): cesx_mh_hmc_lineal_begin (noise, kick, drift), cesx_forward_apply,
                                     cesx_mh_hmc_lineal_leap (gradient, kick, drift), cesx_mh_hmc_lineal_accept (gradient, score)
              hmc_us = {L: us}       the whole step at L leapfrogs
              model_us = {L: us}     the cost model t(L) = lv_us + (L - 1) (forward + leap), beside the measured times
              accept = {L: rate}
    ess     per dtype and start at --ess-M chains: accept rate, the smallest ``summary['ess']`` over the parameters and that per
            second of device time (steps x the step's device time above) for the random walk, MALA and HMC at each L
    adapt   per dtype: ``adapt=--adapt`` from the textbook step, started from the ensemble mean, for update='langevin' and
            update='hmc' at the largest L: the multiplier found, delta', and the accept rate of the steps behind the phase
    clock_ghz   the in-kernel clock class of the box (cesx_calibrate_mfma)
Nothing of this enters bench.py's value and nothing is asserted.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lineal_langevin_bench import problem  # noqa: E402


def _rec():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def time_steps(eng, model, U, L, reps, first, pieces=False):
    """Device us per step over ``reps`` whole steps from step index ``first`` (L = 0: the Langevin step), after 5 warm-up steps;
    ``pieces``: {entry point: us per call} from event pairs around each call instead."""
    import torch
    p, n = eng.p, eng.n_obs
    Q, Q2, GQ = eng.empty(p), eng.empty(p), eng.empty(n)

    def step(k, marks=None):
        ev = (lambda name: marks.append((name, _rec()))) if marks is not None else (lambda name: None)
        q, nxt = Q, Q2
        ev("begin")
        if L == 0:
            eng.mh_langevin_lineal_propose(k, U, out=q)
        else:
            eng.mh_hmc_lineal_begin(k, U, out=q)
        for _ in range(max(L, 1) - 1):
            ev("forward")
            model.forward_device(eng, q, out=GQ)
            ev("leap")
            eng.mh_hmc_lineal_leap(q, GQ, nxt)
            q, nxt = nxt, q
        ev("forward")
        model.forward_device(eng, q, out=GQ)
        ev("accept")
        if L == 0:
            eng.mh_langevin_lineal_accept(k, U, q, GQ)
        else:
            eng.mh_hmc_lineal_accept(k, U, q, GQ)
        ev("end")

    for k in range(5):
        step(first + k)
    torch.cuda.synchronize()
    if not pieces:
        a = _rec()
        for k in range(reps):
            step(first + 5 + k)
        b = _rec()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / reps, 2)
    tot, cnt = {}, {}
    for k in range(reps):
        marks = []
        step(first + 5 + k, marks)
        torch.cuda.synchronize()
        for (name, e0), (_, e1) in zip(marks[:-1], marks[1:]):
            tot[name] = tot.get(name, 0.0) + e0.elapsed_time(e1) * 1e3
            cnt[name] = cnt.get(name, 0) + 1
    return {k: round(tot[k] / cnt[k], 2) for k in tot}


def main():
    import torch
    from scipy import stats
    from ces_amd import calibrate, engine, sample, utils
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=256)
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    ap.add_argument("--L", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ess-M", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--starts", nargs="+", default=["mean", "ensemble"])
    ap.add_argument("--adapt", type=int, default=100)
    args = ap.parse_args()
    p = args.p
    A, Gamma, Sigma, mu, y, ens = problem(p)
    chol = np.linalg.cholesky(np.cov(ens))
    delta = {"rw": 2.38 / np.sqrt(p), "lv": 1.65 * p ** (-1.0 / 6.0)}
    model = utils.lineal(A).enable_gradient(leapfrog=True)
    out = dict(p=p, delta={k: round(v, 4) for k, v in delta.items()}, rows=[], ess=[], adapt=[])
    ghz, step_us = 0.0, {}
    rng = np.random.default_rng(1)
    for M in args.M:
        U0 = ens[:, rng.integers(0, ens.shape[1], M)]
        for dtype in args.dtypes:
            row = dict(M=M, dtype=dtype, reps=args.reps)
            # the random walk, for the ESS rows
            eng = engine.Engine(p, p, M, dtype=dtype)
            eng.set_problem(y, Gamma, mu, Sigma, mu)
            eng.mh_set_proposal(None, delta["rw"] * chol)
            U = eng.to_device(U0, p, "U").clone()
            P, GP = eng.empty(p), eng.empty(p)
            eng.mh_start(U, model.forward_device(eng, U).clone())

            def rw(k):
                eng.mh_propose(k, U, out=P)
                model.forward_device(eng, P, out=GP)
                eng.mh_accept(k, U, P, GP)
            for k in range(5):
                rw(k)
            torch.cuda.synchronize()
            a = _rec()
            for k in range(args.reps):
                rw(5 + k)
            b = _rec()
            torch.cuda.synchronize()
            row["rw_us"] = round(a.elapsed_time(b) * 1e3 / args.reps, 2)
            eng.close()
            # the Langevin and the leapfrog steps on one engine
            eng = engine.Engine(p, p, M, dtype=dtype)
            eng.set_problem(y, Gamma, mu, Sigma, mu)
            eng.mh_set_proposal("hmc", delta["lv"] * chol)
            U = eng.to_device(U0, p, "U").clone()
            model.langevin_device(eng)
            eng.mh_langevin_lineal_start(U, model.forward_device(eng, U).clone())
            first, span = 0, args.reps + 5
            row["lv_us"] = time_steps(eng, model, U, 0, args.reps, first)
            first += span
            row["pieces"] = time_steps(eng, model, U, 2, args.reps, first, pieces=True)
            first += span
            row["hmc_us"], row["accept"] = {}, {}
            for L in args.L:
                before = eng.mh_stats(per_chain=True)[2].sum()
                row["hmc_us"][str(L)] = time_steps(eng, model, U, L, args.reps, first)
                row["accept"][str(L)] = round(float(eng.mh_stats(per_chain=True)[2].sum() - before) / (span * M), 4)
                first += span
            row["lv_us_again"] = time_steps(eng, model, U, 0, args.reps, first)
            per_leap = row["pieces"]["forward"] + row["pieces"]["leap"]
            row["model_us"] = {str(L): round(row["lv_us"] + (L - 1) * per_leap, 2) for L in args.L}
            _, ghz = eng.calibrate_mfma()
            eng.close()
            step_us[(M, dtype)] = row
            out["rows"].append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    # mixing: the smallest ESS per second of device time on the same Gaussian problem
    prior = stats.multivariate_normal(mean=mu, cov=Sigma)
    enka = calibrate.enka(p, p, ens.shape[1])
    enka.Ustar = ens
    M = args.ess_M

    def sampler(dtype):
        mc = sample.MCMC()
        mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", dtype
        return mc
    for dtype in args.dtypes:
        if (M, dtype) not in step_us:
            continue
        t = step_us[(M, dtype)]
        runs = [("rw", dict(update=None, fused=False), delta["rw"], t["rw_us"]), ("lv", dict(update="langevin"), delta["lv"], t["lv_us"])]
        runs += [("hmc%d" % L, dict(update="hmc", leapfrog=L), delta["lv"], t["hmc_us"][str(L)]) for L in args.L]
        for start in args.starts:
            row = dict(M=M, dtype=dtype, start=start, steps=args.steps, burn=args.burn)
            for tag, kw, d, us in runs:
                mc = sampler(dtype)
                mc.model_mh(model, args.steps, prior, enka, Gamma, delta=d, chains=M, summary=True, burn=args.burn, start=start, **kw)
                ess = float(np.min(mc.summary["ess"]))
                ok = bool(np.isfinite(ess))                # (no chain moved: no variance, no ess -- null in the JSON line)
                row.update({"accept_%s" % tag: round(float(mc.accept), 4), "ess_%s" % tag: round(ess, 1) if ok else None,
                            "ess_per_s_%s" % tag: round(ess / (args.steps * us * 1e-6), 1) if ok else None})
                mc._mh_eng.close()
            out["ess"].append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
        # adapt= from the textbook step, every chain from the ensemble mean
        for kw in (dict(update="langevin"), dict(update="hmc", leapfrog=max(args.L))):
            mc = sampler(dtype)
            mc.model_mh(model, args.adapt + args.steps, prior, enka, Gamma, delta=delta["lv"], chains=M, adapt=args.adapt,
                        start="mean", summary=True, burn=args.adapt + args.burn, **kw)
            row = dict(M=M, dtype=dtype, adapt=args.adapt, steps_after=args.steps, multiplier=round(mc.adapt["multiplier"], 4),
                       delta=round(mc.adapt["delta"], 4), accept_first=round(float(mc.adapt["accept_history"][0]), 4),
                       accept_after=round(float(mc.accept), 4), ess_after=round(float(np.min(mc.summary["ess"])), 1), **kw)
            mc._mh_eng.close()
            out["adapt"].append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    out["clock_ghz"] = round(ghz, 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
