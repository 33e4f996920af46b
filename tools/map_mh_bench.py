#!/usr/bin/env python3
"""Price the fused chain kernel of MCMC.model_mh (cesx_mh_run_map: K Metropolis steps per launch, one chain per lane) against
the step path (propose / forward_device / accept: three launches per step and more) and against the host chain, on the
elliptic problem of the reference's notebook (examples/notebooks/elliptic.ipynb).

    python tools/map_mh_bench.py [--M 1024 65536] [--steps 1000] [--dtype float64 float32] [--host-steps 1000]

Problem: ces_amd.utils.elliptic, y = (27.4519.., 79.7019..), Gamma = 0.1^2 I, the prior N(0, 100 I); random walk with
``delta chol(cov(Ustar))`` of a 50-particle ensemble around the posterior; ``noise='device'``, every chain started from an
ensemble member (``start='ensemble'``, the ensemble resampled to M columns), ``trace_stride`` = steps (the first and the last
state cross to the host: the copy of a full trace is the same for both paths and not what is compared).
Prints one JSON line:
    step_ms, fused_ms     per dtype and M: wall time of one ``model_mh`` call of `steps` steps (the second of two calls:
                          the first pays the engine and the allocations), fused=False / fused=True
    us_per_step           the same per step
    ratio                 step_ms / fused_ms
    accept                the overall accept rate of the fused run (equal to the step path's: the same chains)
    host_one_chain_ms     the host ``model_mh`` (no ``chains=``), `host-steps` steps of ONE chain, scaled to `steps`
    clock_ghz             the in-kernel clock class of the box (cesx_calibrate_mfma)
    fused_default_ok      fused_ms <= step_ms at the largest M for every dtype: what MCMC.FUSED_DEFAULT = True stands on; the
                          tool exits with status 1 when it does not hold
Nothing of this enters bench.py's value.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Y = np.array([27.45194112300398, 79.70194112300398])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--dtype", nargs="+", default=["float64", "float32"])
    ap.add_argument("--host-steps", type=int, default=1000)
    args = ap.parse_args()
    import torch
    from scipy import stats
    from ces_amd import calibrate, sample, utils
    Gamma = 0.1 ** 2 * np.identity(2)
    prior = stats.multivariate_normal(mean=np.zeros(2), cov=100.0 * np.identity(2))
    model = utils.elliptic()
    rng = np.random.RandomState(0)
    cloud = np.vstack([-2.65 + 0.07 * rng.standard_normal(50), 104.5 + 0.25 * rng.standard_normal(50)])
    out = dict(step_ms={}, fused_ms={}, us_per_step={}, ratio={}, accept={})
    ghz, ok = 0.0, True
    for dtype in args.dtype:
        for M in args.M:
            enka = calibrate.enka(2, 2, M)
            enka.Ustar = cloud[:, rng.randint(0, 50, M)]
            key = "%s/%d" % (dtype, M)
            ms = {}
            for fused in (False, True):
                mc = sample.MCMC()
                mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype, mc.trace_stride = True, Y, "device", dtype, args.steps
                for rep in range(2):
                    mc.__dict__.pop("samples", None)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    mc.model_mh(model, args.steps, prior, enka, Gamma, delta=1.0, chains=M,
                                start="ensemble", fused=fused)
                    torch.cuda.synchronize()
                    ms[fused] = (time.perf_counter() - t0) * 1e3
                acc = float(mc.accept)
                _, ghz = mc._mh_eng.calibrate_mfma()
                mc._mh_eng.close()
            out["step_ms"][key], out["fused_ms"][key] = round(ms[False], 2), round(ms[True], 2)
            out["us_per_step"][key] = dict(step=round(ms[False] * 1e3 / args.steps, 2), fused=round(ms[True] * 1e3 / args.steps, 3))
            out["ratio"][key] = round(ms[False] / ms[True], 1)
            out["accept"][key] = round(acc, 3)
            if M == max(args.M):
                ok = ok and ms[True] <= ms[False]
    # the host chain: one chain, the reference's loop
    enka = calibrate.enka(2, 2, 50)
    enka.Ustar = cloud
    host = sample.MCMC()
    host.mute_bar, host.y_obs = True, Y
    np.random.seed(0)
    t0 = time.perf_counter()
    host.model_mh(model, args.host_steps, prior, enka, Gamma, delta=1.0)
    host_ms = (time.perf_counter() - t0) * 1e3 * args.steps / max(1, args.host_steps)
    out.update(shape=dict(M=args.M, steps=args.steps, dtype=args.dtype), host_one_chain_ms=round(host_ms, 1),
               host_accept=round(float(host.accept), 3), clock_ghz=round(ghz, 3), fused_default_ok=bool(ok))
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
