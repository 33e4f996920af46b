#!/usr/bin/env python3
"""Time the GP emulator on the device (cesx_gp_*) at benchmark shape E1.

    python tools/gp_bench.py [--chains 65536] [--p 8] [--n 32] [--jt 512] [--steps 50] [--warmup 5] [--cpu]

65 536 chains, p = 8, 32 GPs (n_obs), J_t = 512 training points, Matern-3/2 ARD, Gamma None (the variance is needed),
random walk, device noise, fp64 engine.  Prints one JSON line: ms per gp_mh step (propose + predict + accept), ms per
predict with and without the variance, and the fraction of the fp64 MFMA peak (78.2 TF) on the triangular flops
n M J_t (J_t + 1) / 2 MACs.  The kernel split comes from ``rocprofv3 --kernel-trace --stats -- python tools/gp_bench.py``.
--cpu also times the vectorised numpy predict of the same step on the host for context.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_MFMA = 78.2e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--jt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    p, n, M, Jt = args.p, args.n, args.chains, args.jt
    rng = np.random.default_rng(0)
    U = rng.standard_normal((p, Jt))
    gps = []
    for i in range(n):
        y = np.sin(U[i % p]) + 0.1 * U.sum(0)
        m = em.GPR(U.T, y[:, None], em.Matern32(input_dim=p, ARD=True, lengthscales=1.5 + rng.random(p)),
                   mean_function=em.Linear(0.1 * rng.standard_normal((p, 1)), [0.0]))
        m.likelihood.variance = 1e-4
        gps.append(m)

    class E(object):
        pass
    enka = E()
    enka.p, enka.n_obs, enka.Ustar, enka.gpmodels = p, n, U, gps
    t0 = time.perf_counter()
    img = em.device_image(enka, gps)
    t_img = time.perf_counter() - t0
    eng = engine.Engine(p, n, M, dtype="float64")
    y = np.zeros(n)
    eng.set_problem(y, np.eye(n), np.zeros(p), np.eye(p), np.zeros(p))
    eng.mh_set_proposal(None, 0.05 * np.eye(p))
    eng.gp_set(img)
    X = eng.to_device(0.5 * rng.standard_normal((p, M)), p).clone()
    P = eng.empty(p)
    mean = torch.empty((n, M), dtype=torch.float64, device=eng.device)
    var = torch.empty_like(mean)

    def timed(fn, k):
        for _ in range(args.warmup):
            fn(0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s in range(k):
            fn(s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / k * 1e3

    ms_var = timed(lambda s: eng.gp_predict(X, var=True, out=(mean, var)), args.steps)
    ms_mean = timed(lambda s: eng.gp_predict(X, var=False, out=(mean, None)), args.steps)
    eng.gp_predict(X, out=(mean, var))
    eng.gp_start("var", X, mean, var)

    def step(s):
        eng.mh_propose(s, X, out=P)
        eng.gp_predict(P, out=(mean, var))
        eng.gp_accept("var", s, X, P, mean, var)
    ms_step = timed(step, args.steps)
    flops = 2.0 * n * M * Jt * (Jt + 1) / 2
    out = dict(shape=dict(chains=M, p=p, n_gp=n, J_t=Jt, kernel="Matern32"), ms_per_step=ms_step,
               ms_predict_var=ms_var, ms_predict_mean=ms_mean, mfma_peak_fraction=flops / (ms_var * 1e-3) / PEAK_F64_MFMA,
               host_image_s=t_img)
    if args.cpu:
        Xh = eng.to_host(X)[:, :4096]
        t = time.perf_counter()
        for m in gps:
            m.predict_y(Xh.T)
        out["ms_numpy_predict_per_4096_chains"] = (time.perf_counter() - t) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
