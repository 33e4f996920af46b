#!/usr/bin/env python3
"""Time one Metropolis-Hastings step of the device path (cesx_mh_*) at the benchmark's shape.

    python tools/mh_bench.py [--chains 65536] [--p 256] [--steps 200] [--warmup 20] [--cpu]

65 536 chains, p = n_obs = 256, fp32, utils.lineal, random walk, diagonal Gamma and Sigma, device noise.  Prints ms per
MH step (propose + forward map + accept, host clock around a synchronised window) and chain-steps/s.  The kernel split
comes from a separate run under ``rocprofv3 --kernel-trace --stats -- python tools/mh_bench.py`` (its stats name
update2_kernel twice per step -- the proposal with in-kernel noise, the forward map -- and mh_accept_kernel once).
--cpu also times the vectorised numpy restatement of the same step on the host's cores for context.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--p", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from ces_amd import engine
    p = n = args.p
    M = args.chains
    rng = np.random.default_rng(0)
    A = rng.standard_normal((n, p)) / np.sqrt(p)
    gam = np.full(n, 0.1)
    y = A @ (0.5 * rng.standard_normal(p)) + np.sqrt(gam) * rng.standard_normal(n)
    mu, sig = np.zeros(p), np.ones(p)
    S = np.sqrt(2 * 0.15 / n) * np.eye(p)
    eng = engine.Engine(p, n, M, dtype="float32")
    eng.set_problem(y, np.diag(gam), mu, np.diag(sig), mu)
    eng.forward_set_lineal(A)
    eng.mh_set_proposal(None, S)
    U = eng.to_device(0.3 * rng.standard_normal((p, M)), p).clone()
    G, P, GP = eng.empty(n), eng.empty(p), eng.empty(n)
    eng.forward_apply(U, out=G)
    eng.mh_start(U, G)

    def step(k):
        eng.mh_propose(k, U, out=P)
        eng.forward_apply(P, out=GP)
        eng.mh_accept(k, U, P, GP)

    for k in range(args.warmup):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.warmup, args.warmup + args.steps):
        step(k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    _, rate = eng.mh_stats()
    esz = 4
    out = dict(chains=M, p=p, n_obs=n, dtype="float32", steps=args.steps, ms_per_step=dt * 1e3,
               chain_steps_per_s=M / dt, accept=rate,
               accept_bytes_min=int(M * esz * (n + p) + M * 8 * 2 + rate * M * esz * 2 * p))
    if args.cpu:
        Xh = 0.3 * rng.standard_normal((p, M))
        phi = 0.5 * (((A @ Xh - y[:, None]) ** 2) / gam[:, None]).sum(0) + 0.5 * (Xh ** 2).sum(0)
        t0 = time.perf_counter()
        for _ in range(3):
            Ph = Xh + S @ rng.standard_normal((p, M))
            pp = 0.5 * (((A @ Ph - y[:, None]) ** 2) / gam[:, None]).sum(0) + 0.5 * (Ph ** 2).sum(0)
            acc = np.log(rng.random(M)) < phi - pp
            Xh[:, acc] = Ph[:, acc]
            phi[acc] = pp[acc]
        out["cpu_numpy_ms_per_step"] = (time.perf_counter() - t0) / 3 * 1e3
        out["cpu_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
