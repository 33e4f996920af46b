#!/usr/bin/env python3
"""Price a step of the Darcy chains of MCMC.model_mh(chains=M): the random walk against Langevin and leapfrog HMC on the adjoint
launch (cesx_darcy_grad + the cesx_mh_langevin_* / cesx_mh_hmc_* entry points under cesx_mh_grad_source(READY)).

    python tools/darcy_chain_bench.py [--K 16] [--p 64] [--n 50] [--Js 1024,8192] [--steps 20] [--warmup 3] [--dtype float64]

Built on tools/darcy_grad_bench.py (its problem, its timer: HIP events around `steps` back-to-back steps, device noise, nothing
read back inside the window).  Prints one JSON line per J:
    rw_ms, langevin_ms, hmc2_ms, hmc4_ms   device time of ONE step of all chains: the forward launch + cesx_mh_propose / _accept;
                                           propose + adjoint + accept; begin + L adjoints + (L - 1) leaps + accept, L = 2 and 4
    apply_ms, grad_ms                      one cesx_darcy_apply / one cesx_darcy_grad of the chains
    propose_ms, score_ms, leap_ms          one cesx_mh_langevin_propose; one scoring launch (dc_lv_accept_kernel: phi, g, the test)
                                           and one leap launch (dc_hm_leap_kernel) on fixed G and d
    model_langevin, model_hmc(L)           the expectation to check: grad + propose + score, langevin + (L - 1) (grad + leap)
    clock_ghz                              the shader clock of a bare MFMA loop on this device just before the window
Nothing of this enters bench.py's value, and nothing is gated on it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from darcy_grad_bench import timed  # noqa: E402


def steps(args, J):
    import torch
    from ces_amd import darcy, engine
    K, n, p = args.K, args.n, args.p
    rng = np.random.default_rng(0)
    mdl = darcy.model_trunc(Nmesh=float(K), p=p) if p < K * K else darcy.model(Nmesh=float(K))
    mdl.obs_index = rng.choice(K * K, n, replace=False)
    mdl.enable_gradient()
    truth = rng.standard_normal(p)
    g0 = mdl(truth)
    sd = 0.05 * np.max(np.abs(g0))
    y, Gamma = g0 + sd * rng.standard_normal(n), sd * sd * np.eye(n)
    eng = engine.Engine(p, n, J, dtype=args.dtype)
    eng.set_problem(y, Gamma, np.zeros(p), np.eye(p), np.zeros(p))
    Uh = truth[:, None] + 0.3 * rng.standard_normal((p, J))
    S = 0.05 * np.linalg.cholesky(np.cov(Uh))
    U = eng.to_device(Uh, p, "U").clone()
    P, G = eng.empty(p), eng.empty(n)
    status = torch.zeros(J, dtype=torch.int32, device=eng.device)
    mdl.forward_device(eng, U, out=G)                       # installs the map
    out = mdl.gradient_device(eng, U)
    _, clock = eng.calibrate_mfma()
    res = dict(clock_ghz=clock)
    k = [0]

    def apply(X=U):
        eng._check(eng.lib.cesx_darcy_apply(eng._h, X.data_ptr(), G.data_ptr(), status.data_ptr(), eng._stream()))

    def grad(X):
        eng.darcy_grad(X, out=out)
        return out[0], out[2]

    # the random walk: propose, the forward launch, accept
    eng.mh_set_proposal(None, S)
    apply()
    eng.mh_start(U, G)

    def rw():
        k[0] += 1
        eng.mh_propose(k[0], U, out=P)
        apply(P)
        eng.mh_accept(k[0], U, P, G)
    res["rw_ms"] = timed(torch, rw, args.steps, args.warmup)
    res["rw_accept"] = eng.mh_stats()[1]

    # Langevin and HMC on the adjoint launch
    eng.mh_set_proposal("langevin", S)
    eng.mh_grad_source("ready")
    eng.mh_langevin_start(U, *grad(U))

    def langevin():
        k[0] += 1
        eng.mh_langevin_propose(k[0], U, out=P)
        eng.mh_langevin_accept(k[0], U, P, *grad(P))

    def hmc(L):
        def step():
            k[0] += 1
            eng.mh_hmc_begin(k[0], U, out=P)
            for _ in range(L - 1):
                eng.mh_hmc_leap(P, *grad(P))
            eng.mh_hmc_accept(k[0], U, P, *grad(P))
        return step
    res["langevin_ms"] = timed(torch, langevin, args.steps, args.warmup)
    res["langevin_accept"] = eng.mh_stats()[1]
    res["hmc2_ms"] = timed(torch, hmc(2), args.steps, args.warmup)
    res["hmc4_ms"] = timed(torch, hmc(4), args.steps, args.warmup)
    # the pieces, one launch each on fixed inputs (log u = -inf never accepts: U, phi and g stay what they are)
    res["apply_ms"] = timed(torch, apply, args.steps, args.warmup)
    res["grad_ms"] = timed(torch, lambda: grad(U), args.steps, args.warmup)
    never = torch.full((J,), -np.inf, dtype=torch.float64, device=eng.device)
    res["propose_ms"] = timed(torch, lambda: eng.mh_langevin_propose(1, U, out=P), args.steps, args.warmup)
    Gd = grad(P)

    def score():
        eng.mh_langevin_propose(1, U, out=P)
        eng.mh_langevin_accept(1, U, P, *Gd, logu=never)
    res["score_ms"] = timed(torch, score, args.steps, args.warmup) - res["propose_ms"]
    Q = P.clone()

    def leap():
        eng.mh_hmc_begin(1, U, out=Q)
        eng.mh_hmc_leap(Q, *Gd)
    begin_ms = timed(torch, lambda: eng.mh_hmc_begin(1, U, out=Q), args.steps, args.warmup)
    res["leap_ms"] = timed(torch, leap, args.steps, args.warmup) - begin_ms
    res["model_langevin"] = res["grad_ms"] + res["propose_ms"] + res["score_ms"]
    for L in (2, 4):
        res["model_hmc%d" % L] = res["model_langevin"] + (L - 1) * (res["grad_ms"] + res["leap_ms"])
    res["score_share_of_langevin"] = res["score_ms"] / res["langevin_ms"]
    eng.close()
    return dict(shape=dict(K=K, p=p, n_obs=n, J=J, dtype=args.dtype), **{k_: round(float(v), 4) for k_, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--p", type=int, default=64)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--Js", default="1024,8192")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="float64")
    args = ap.parse_args()
    for J in [int(v) for v in args.Js.split(",")]:
        print(json.dumps(steps(args, J)), flush=True)


if __name__ == "__main__":
    main()
