#!/usr/bin/env python3
"""Price the Langevin step of MCMC.model_mh(chains=M, update='langevin') on the linear map at the benchmark's shape
(p = n_obs = 256) against the random-walk step of the same build, in the same process, on the same box, in the same run.

    python tools/lineal_langevin_bench.py [--p 256] [--M 1024 65536] [--dtypes float32 float64] [--reps 50]
                                          [--ess-M 1024] [--steps 400] [--burn 100] [--starts mean ensemble]

The problem is Gaussian: A = randn / sqrt(p), Gamma = 0.1^2 I, Sigma = I, mu = 0, a 1 024-particle ensemble of exact posterior
draws for the scales.  The steps are the textbook scalings and are not tuned: random walk delta = 2.38 / sqrt(p), Langevin
delta = 1.65 p^(-1/6).
Prints one JSON line:
    rows    per M / dtype, in microseconds of DEVICE time per step (hip events on the stream; ``*_us``: one event pair around
            ``reps`` whole steps; ``*_split``: pairs around each entry point, which adds the markers' own gaps):
              rw_us, rw_split = {propose, forward, accept}                   cesx_mh_propose / cesx_forward_apply / cesx_mh_accept
              lv_us, lv_split = {propose, forward, accept}                   cesx_mh_langevin_lineal_propose (noise draw, z, the
                                                                             triangular launch) / cesx_forward_apply /
                                                                             cesx_mh_langevin_lineal_accept (the gradient launch and
                                                                             lvlin_accept_kernel)
              ratio = lv_us / rw_us
    ess     per dtype and start at --ess-M chains (``start='mean'``: every chain from the ensemble mean, so the run includes the
            way out of the mode; ``start='ensemble'``: from exact posterior draws, the stationary regime the scalings are
            stated for; needs --ess-M <= 1 024): accept rate, the smallest ``summary['ess']`` over the parameters and that
            per second of device time (steps x the step's device time above) for both samplers
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


def problem(p, n_ens=1024):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((p, p)) / np.sqrt(p)
    Gamma, Sigma, mu = 0.1 ** 2 * np.eye(p), np.eye(p), np.zeros(p)
    y = A @ rng.standard_normal(p) + 0.1 * rng.standard_normal(p)
    C = np.linalg.inv(A.T @ A / 0.1 ** 2 + np.eye(p))
    C = 0.5 * (C + C.T)
    m = C @ (A.T @ y / 0.1 ** 2)
    ens = m[:, None] + np.linalg.cholesky(C) @ rng.standard_normal((p, n_ens))
    return A, Gamma, Sigma, mu, y, ens


def time_steps(eng, model, U, langevin, reps):
    """(device us per step over ``reps`` whole steps, {entry point: us per step})."""
    import torch
    p, n = eng.p, eng.n_obs
    P, GP = eng.empty(p), eng.empty(n)

    def step(k, marks=None):
        ev = (lambda: marks.append(_rec())) if marks is not None else (lambda: None)
        ev()
        if langevin:
            eng.mh_langevin_lineal_propose(k, U, out=P)
        else:
            eng.mh_propose(k, U, out=P)
        ev()
        model.forward_device(eng, P, out=GP)
        ev()
        if langevin:
            eng.mh_langevin_lineal_accept(k, U, P, GP)
        else:
            eng.mh_accept(k, U, P, GP)
        ev()

    def _rec():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    for k in range(5):
        step(k)
    torch.cuda.synchronize()
    a = _rec()
    for k in range(reps):
        step(5 + k)
    b = _rec()
    torch.cuda.synchronize()
    whole = a.elapsed_time(b) * 1e3 / reps
    split = dict(propose=0.0, forward=0.0, accept=0.0)
    for k in range(reps):
        marks = []
        step(5 + reps + k, marks)
        torch.cuda.synchronize()
        for name, i in (("propose", 0), ("forward", 1), ("accept", 2)):
            split[name] += marks[i].elapsed_time(marks[i + 1]) * 1e3 / reps
    return round(whole, 2), {k: round(v, 2) for k, v in split.items()}


def main():
    from scipy import stats
    from ces_amd import calibrate, engine, sample, utils
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=256)
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ess-M", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--starts", nargs="+", default=["mean", "ensemble"])
    args = ap.parse_args()
    p = args.p
    A, Gamma, Sigma, mu, y, ens = problem(p)
    chol = np.linalg.cholesky(np.cov(ens))
    delta = {"rw": 2.38 / np.sqrt(p), "lv": 1.65 * p ** (-1.0 / 6.0)}
    model = utils.lineal(A).enable_gradient()
    out, ghz, step_us = dict(p=p, delta={k: round(v, 4) for k, v in delta.items()}, rows=[], ess=[]), 0.0, {}
    rng = np.random.default_rng(1)
    for M in args.M:
        U0 = ens[:, rng.integers(0, ens.shape[1], M)]
        for dtype in args.dtypes:
            row = dict(M=M, dtype=dtype, reps=args.reps)
            for tag, update in (("rw", None), ("lv", "langevin")):
                eng = engine.Engine(p, p, M, dtype=dtype)
                eng.set_problem(y, Gamma, mu, Sigma, mu)
                eng.mh_set_proposal(update, delta[tag] * chol)
                U = eng.to_device(U0, p, "U").clone()
                G = model.forward_device(eng, U).clone()
                if update:
                    model.langevin_device(eng)
                    eng.mh_langevin_lineal_start(U, G)
                else:
                    eng.mh_start(U, G)
                row["%s_us" % tag], row["%s_split" % tag] = time_steps(eng, model, U, bool(update), args.reps)
                row["accept_%s" % tag] = round(eng.mh_stats()[1], 4)
                _, ghz = eng.calibrate_mfma()
                eng.close()
            row["ratio"] = round(row["lv_us"] / row["rw_us"], 3)
            step_us[(M, dtype)] = (row["rw_us"], row["lv_us"])
            out["rows"].append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    # mixing: the smallest ESS per second of device time, both samplers, on the same Gaussian problem
    prior = stats.multivariate_normal(mean=mu, cov=Sigma)
    enka = calibrate.enka(p, p, ens.shape[1])
    enka.Ustar = ens
    M = args.ess_M
    for dtype in args.dtypes:
        if (M, dtype) not in step_us:
            continue
        for start in args.starts:
            row = dict(M=M, dtype=dtype, start=start, steps=args.steps, burn=args.burn)
            for i, (tag, update) in enumerate((("rw", None), ("lv", "langevin"))):
                mc = sample.MCMC()
                mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", dtype
                mc.model_mh(model, args.steps, prior, enka, Gamma, delta=delta[tag], chains=M, update=update, fused=False,
                            summary=True, burn=args.burn, start=start)
                ess = float(np.min(mc.summary["ess"]))
                dev_s = args.steps * step_us[(M, dtype)][i] * 1e-6
                row.update({"accept_%s" % tag: round(float(mc.accept), 4), "ess_%s" % tag: round(ess, 1),
                            "ess_per_s_%s" % tag: round(ess / dev_s, 1)})
                mc._mh_eng.close()
            out["ess"].append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    out["clock_ghz"] = round(ghz, 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
