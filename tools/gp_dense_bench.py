#!/usr/bin/env python3
"""Time the dense per-chain likelihood of gp_mh(chains=, pca_tools=) (cesx_gp_dense_set, gp_score_dense_kernel).

    python tools/gp_dense_bench.py [--p 4] [--jt 256] [--reps 20] [--warmup 3] [--host-steps 200]

For (n, k, M) = (50, 8, 65 536) and (128, 16, 8 192): the score launch (gp_accept in mode 'dense') beside gp_predict of the
k GPs (mean and variance), and the whole device step (propose + predict + score), each timed with HIP events around
``reps`` launches.  For the bar, (50, 8, 4 096): one device step against 4 096 single-chain steps of the host gp_mh on
this box (``host-steps`` steps timed, scaled).  Prints one JSON line per shape and one for the bar; the shader clock comes
from the engine's in-kernel clock calibration (cesx_calibrate_mfma) before and after.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Enka(object):
    pass


def problem(rng, p, n, k, Jt):
    from ces_amd import emulate as em
    U = rng.standard_normal((p, Jt))
    gps = []
    for i in range(k):
        y = np.sin(U[i % p]) + 0.1 * U.sum(0) + 0.05 * i
        m = em.GPR(U.T, y[:, None], em.Matern32(input_dim=p, ARD=True, lengthscales=1.5 + rng.random(p)),
                   mean_function=em.Linear(0.1 * rng.standard_normal((p, 1)), [0.0]))
        m.likelihood.variance = 1e-4
        gps.append(m)
    enka = Enka()
    enka.p, enka.n_obs, enka.Ustar, enka.gpmodels = p, n, U, gps
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    Gamma = 0.01 * (Q * np.exp(np.linspace(0.0, -np.log(1e3), n))) @ Q.T
    Gamma = (Gamma + Gamma.T) / 2
    VD_k = np.linalg.qr(rng.standard_normal((n, k)))[0] * np.exp(rng.uniform(-1.0, 0.0, k))
    mG = 0.1 * rng.standard_normal((n, 1))
    y_obs = mG.ravel() + 0.1 * rng.standard_normal(n)
    return enka, Gamma, VD_k, mG, y_obs


def events_ms(torch, fn, reps, warmup):
    for s in range(warmup):
        fn(s)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for s in range(reps):
        fn(s)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def device_times(args, n, k, M, rng):
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    p = args.p
    enka, Gamma, VD_k, mG, y_obs = problem(rng, p, n, k, args.jt)
    eng = engine.Engine(p, n, M, dtype="float64")
    _, ghz0 = eng.calibrate_mfma()
    eng.set_problem(y_obs, Gamma, np.zeros(p), np.eye(p), np.zeros(p))
    eng.mh_set_proposal(None, 0.05 * np.eye(p))
    eng.gp_set(em.device_image(enka, enka.gpmodels))
    eng.gp_dense_set(VD_k, mG, True)
    X = eng.to_device(0.5 * rng.standard_normal((p, M)), p).clone()
    P = eng.empty(p)
    mean = torch.empty((k, M), dtype=torch.float64, device=eng.device)
    var = torch.empty_like(mean)
    eng.gp_predict(X, out=(mean, var))
    eng.gp_start("dense", X, mean, var)
    eng.mh_propose(0, X, out=P)
    ms_predict = events_ms(torch, lambda s: eng.gp_predict(P, out=(mean, var)), args.reps, args.warmup)
    ms_score = events_ms(torch, lambda s: eng.gp_accept("dense", s, X, P, mean, var), args.reps, args.warmup)

    def step(s):
        eng.mh_propose(s, X, out=P)
        eng.gp_predict(P, out=(mean, var))
        eng.gp_accept("dense", s, X, P, mean, var)
    ms_step = events_ms(torch, step, args.reps, args.warmup)
    _, ghz1 = eng.calibrate_mfma()
    _, rate = eng.mh_stats()
    return dict(shape=dict(n=n, k=k, chains=M, p=p, J_t=args.jt), ms_score=ms_score, ms_predict=ms_predict, ms_step=ms_step,
                us_score_per_chain=1e3 * ms_score / M, accept_rate=rate, shader_ghz=[ghz0, ghz1])


def host_ms_per_step(args, n, k, rng):
    from scipy import stats
    from ces_amd import sample
    p = args.p
    enka, Gamma, VD_k, mG, y_obs = problem(rng, p, n, k, args.jt)
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = y_obs
    prior = stats.multivariate_normal(mean=np.zeros(p), cov=np.eye(p))
    kw = dict(Gamma=Gamma, pca_tools=dict(VD_k=VD_k, mG=mG), noise_compounded=True, delta=0.05, enka_scaling=False)
    np.random.seed(0)
    mc.gp_mh(enka, 5, prior, **kw)
    del mc.samples
    t = time.perf_counter()
    mc.gp_mh(enka, args.host_steps, prior, **kw)
    return (time.perf_counter() - t) / args.host_steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--jt", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=200)
    args = ap.parse_args()
    for n, k, M in ((50, 8, 65536), (128, 16, 8192)):
        print(json.dumps(device_times(args, n, k, M, np.random.default_rng([n, k]))), flush=True)
    n, k, M = 50, 8, 4096
    dev = device_times(args, n, k, M, np.random.default_rng([n, k]))
    host = host_ms_per_step(args, n, k, np.random.default_rng([n, k]))
    print(json.dumps(dict(bar=dict(n=n, k=k, chains=M), ms_device_step=dev["ms_step"], ms_host_step=host,
                          ms_host_4096_steps=host * M, device_step_faster=bool(dev["ms_step"] < host * M),
                          ms_score=dev["ms_score"], ms_predict=dev["ms_predict"], shader_ghz=dev["shader_ghz"])), flush=True)


if __name__ == "__main__":
    main()
