#!/usr/bin/env python3
"""Time the gradient samplers on the projected Sigma (cesx_gp_proj_coef, cesx_gp_proj_langevin_* / cesx_gp_proj_hmc_*;
kernels_gpprojgrad.hip) beside the random walk of the same build.

    python tools/gp_proj_langevin_bench.py [--p 4] [--jt 256] [--reps 20] [--warmup 3] [--rounds 2] [--min-ms 200]
                                           [--ess-steps 64] [--ess-adapt 32] [--ess-chains 4096] [--delta 0.1]

At tools/gp_proj_bench.py's shapes (n, k, M) = (50, 8, 65 536), (128, 16, 8 192) and (180, 16, 65 536), on one engine pair (a
random-walk and a Langevin proposal on the same emulator, descriptor, states and rows), in one process, every timing HIP events
around ``reps`` launches or as many as fill ``min-ms`` milliseconds, the smallest of ``rounds`` reported beside all of them:
  * the coefficient launch (gp_proj_coef, log det on: all five phases; and off: phases 1-3) against the score launch
    (gp_accept in mode 'proj'); ``coef_over_score`` is the ratio the flop model puts near 4;
  * one whole step of every chain: the random walk (propose, predict, accept), the Langevin step (propose, predict with
    gradients, accept) and the leapfrog step at L = 2 and 4 (begin, L predicts with gradients, L - 1 leaps, accept);
  * effective samples per second of gp_mh(chains=, sigma_form='projected', summary=True, autocorr=True) for the four updates,
    ``ess-chains`` chains, ``ess-adapt`` steps left out of the summary (``burn=``) and ``ess-steps`` kept: the random walk at
    ``delta`` as given, the gradient samplers from ``delta`` through ``adapt=ess-adapt`` (the pooled step-size adaptation; the
    step it ends at and the accept rate are reported).  ESS is the smallest over the parameters; it is divided by the wall
    time of the whole call, engine set-up and the left-out steps included.  A sampler that accepts (almost) nothing has no
    ESS worth the name: its entry carries ``stuck``.
Prints one JSON line per shape; the shader clock comes from the engine's in-kernel clock calibration before and after.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gp_dense_bench import problem  # noqa: E402
from gp_proj_bench import timed_ms  # noqa: E402


def device_times(args, n, k, M, rng):
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    p = args.p
    enka, Gamma, VD_k, mG, y_obs = problem(rng, p, n, k, args.jt)
    img = em.device_image(enka, enka.gpmodels)
    proj = em.project_sigma(Gamma, VD_k, mG, y_obs)
    S = 0.05 * np.eye(p)

    def make(kind, logdet=True):
        eng = engine.Engine(p, n, M, dtype="float64")
        eng.set_problem(y_obs, Gamma, np.zeros(p), np.eye(p), np.zeros(p))
        eng.mh_set_proposal(kind, S)
        eng.gp_set(img)
        eng.gp_proj_set(*proj, logdet)
        return eng
    rw, lv = make(None), make("langevin")
    _, ghz0 = lv.calibrate_mfma()
    X = lv.to_device(0.5 * rng.standard_normal((p, M)), p).clone()
    Xr = X.clone()
    P, Pr = lv.empty(p), rw.empty(p)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=lv.device)      # noqa: E731
    rows = (new(k, M), new(k, M), new(k, p, M), new(k, p, M))
    coef_out = (new(M), new(k, M), new(k, M))
    rw.gp_predict(Xr, out=rows[:2])
    rw.gp_start("proj", Xr, *rows[:2])
    lv.gp_predict_grad(X, out=rows)
    lv.gp_langevin_start("proj", X, *rows)

    def rw_step(s):
        rw.mh_propose(s, Xr, out=Pr)
        rw.gp_predict(Pr, out=rows[:2])
        rw.gp_accept("proj", s, Xr, Pr, *rows[:2])

    def lv_step(s):
        lv.gp_langevin_propose(s, X, out=P)
        lv.gp_predict_grad(P, out=rows)
        lv.gp_langevin_accept("proj", s, X, P, *rows)

    def hmc_step(L):
        def step(s):
            lv.mh_hmc_begin(s, X, out=P)
            for _ in range(L - 1):
                lv.gp_predict_grad(P, out=rows)
                lv.gp_hmc_leap("proj", P, *rows)
            lv.gp_predict_grad(P, out=rows)
            lv.gp_hmc_accept("proj", s, X, P, *rows)
        return step
    lv0 = make("langevin", logdet=False)
    parts = dict(score=lambda s: rw.gp_accept("proj", s, Xr, Pr, *rows[:2]),
                 coef=lambda s: lv.gp_proj_coef(rows[0], rows[1], out=coef_out),
                 coef_no_logdet=lambda s: lv0.gp_proj_coef(rows[0], rows[1], out=coef_out),
                 predict=lambda s: rw.gp_predict(Pr, out=rows[:2]),
                 predict_grad=lambda s: lv.gp_predict_grad(P, out=rows),
                 step_rw=rw_step, step_langevin=lv_step, step_hmc2=hmc_step(2), step_hmc4=hmc_step(4))
    rw.mh_propose(0, Xr, out=Pr)
    lv.gp_langevin_propose(0, X, out=P)
    ms = {name: [] for name in parts}
    for _ in range(args.rounds):
        for name, fn in parts.items():
            ms[name].append(timed_ms(torch, fn, args)[0])
    _, ghz1 = lv.calibrate_mfma()
    out = dict(shape=dict(n=n, k=k, chains=M, p=p, J_t=args.jt), shader_ghz=[ghz0, ghz1])
    for name in parts:
        out["ms_" + name] = min(ms[name])
        out["ms_%s_rounds" % name] = ms[name]
    out["coef_over_score"] = out["ms_coef"] / out["ms_score"]
    out["coef_no_logdet_over_score"] = out["ms_coef_no_logdet"] / out["ms_score"]
    for name in ("step_langevin", "step_hmc2", "step_hmc4"):
        out[name + "_over_rw"] = out["ms_" + name] / out["ms_step_rw"]
    out["ess"] = ess_per_second(args, enka, Gamma, VD_k, mG, y_obs, min(M, args.ess_chains))
    return out


def ess_per_second(args, enka, Gamma, VD_k, mG, y_obs, M):
    from scipy import stats
    from ces_amd import sample
    p = enka.p
    prior = stats.multivariate_normal(mean=np.zeros(p), cov=np.eye(p))
    res = {}
    for name, kw in (("rw", {}), ("langevin", dict(update="langevin")), ("hmc2", dict(update="hmc", leapfrog=2)),
                     ("hmc4", dict(update="hmc", leapfrog=4))):
        mc = sample.MCMC()
        mc.mute_bar, mc.y_obs, mc.noise, mc.seed = True, y_obs, "device", 11
        if kw:
            kw["adapt"] = args.ess_adapt
        t0 = time.perf_counter()
        mc.gp_mh(enka, args.ess_adapt + args.ess_steps, prior, delta=args.delta, chains=M, start="mean",
                 pca_tools=dict(VD_k=VD_k, mG=mG), Gamma=Gamma, noise_compounded=True, sigma_form="projected", summary=True,
                 autocorr=True, burn=args.ess_adapt, **kw)
        dt = time.perf_counter() - t0
        ess = float(np.min(mc.autocorr["ess"]))
        res[name] = dict(seconds=dt, accept=float(mc.accept), delta=float(mc.adapt["delta"]) if kw else args.delta,
                         ess_min=ess, ess_per_second=ess / dt, stuck=bool(not mc.accept > 0.01))
    return dict(chains=M, steps=args.ess_steps, adapt=args.ess_adapt, delta=args.delta, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--jt", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--ess-steps", type=int, default=64)
    ap.add_argument("--ess-adapt", type=int, default=32)
    ap.add_argument("--ess-chains", type=int, default=4096)
    ap.add_argument("--delta", type=float, default=0.1)
    args = ap.parse_args()
    for n, k, M in ((50, 8, 65536), (128, 16, 8192), (180, 16, 65536)):
        print(json.dumps(device_times(args, n, k, M, np.random.default_rng([n, k]))), flush=True)


if __name__ == "__main__":
    main()
