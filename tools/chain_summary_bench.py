#!/usr/bin/env python3
"""Price ``summary=True`` (cesx_chain_summary_*: the kept states summed on the device) against what the chain driver did with
the kept states before it existed -- every one copied to the host -- at the two samplers' headline shapes.

    python tools/chain_summary_bench.py [--only elliptic lineal kernels] [--steps 1000] [--lineal-steps 16 40] [--mem]

elliptic   ces_amd.utils.elliptic (the notebook's problem, as tools/map_mh_bench.py sets it up), fused, fp64, `steps` steps,
           65 536 and 1 024 chains, trace_stride 1
lineal     ces_amd.utils.lineal at p = n_obs = 256, 65 536 chains, fp32, the step path (tools/mh_bench.py's problem through
           ``model_mh``): trace_stride 1 over the first and 10 over the second of `lineal-steps` (a kept state is 134 MB on the
           host: a long stride-1 trace does not fit)
Each runs three ways: ``trace`` -- the call as it was, the kept states to the host; ``last`` -- its cheapest form,
``trace_stride = n_mcmc`` (the start and the last state only); ``summary`` -- ``summary=True`` at the trace run's stride.
The first two are the driver's behaviour without this stage: the baseline.  Wall time of the second of two calls (the first
pays the engine and the allocations), per step.  --mem adds the host's peak allocation (tracemalloc: numpy reports to it)
of one more call at `steps` and at `steps` / 2, which shows what grows with n_mcmc.
kernels    the stage's launches alone (device events around ``chain_summary_add``, per draw): the elliptic shape in chunks of
           `steps` draws and the lineal shape draw by draw.  The split by kernel comes from a run of this mode under
           ``rocprofv3 --kernel-trace --stats -- python tools/chain_summary_bench.py --only kernels``.
Prints one JSON line; clock_ghz is the in-kernel clock class of the box (cesx_calibrate_mfma).  Nothing of this enters
bench.py's value.
"""
import argparse
import json
import os
import sys
import time
import tracemalloc

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Y = np.array([27.45194112300398, 79.70194112300398])
MODES = ("last", "summary", "trace")


def timed(mc, call, steps, mode, stride, mem=False):
    import torch
    kw = dict(summary=True) if mode == "summary" else {}
    mc.trace_stride = steps if mode == "last" else stride
    ms = 0.0
    for rep in range(2):
        mc.__dict__.pop("samples", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(steps, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    out = dict(ms=round(ms, 2), us_per_step=round(ms * 1e3 / steps, 2), samples_mb=round(mc.samples.nbytes / 1e6, 1))
    if mem:
        peak = {}
        for n in (steps, steps // 2):
            if mode == "summary" and n // stride < 4:          # (too few draws for the split statistics)
                continue
            mc.__dict__.pop("samples", None)
            if mode == "last":
                mc.trace_stride = n
            tracemalloc.start()
            call(n, **kw)
            peak[n] = tracemalloc.get_traced_memory()[1]
            tracemalloc.stop()
        out["host_peak_mb"] = {str(n): round(v / 1e6, 1) for n, v in peak.items()}
    mc.__dict__.pop("samples", None)
    return out


def elliptic(args, out):
    from scipy import stats
    from ces_amd import calibrate, sample, utils
    Gamma = 0.1 ** 2 * np.identity(2)
    prior = stats.multivariate_normal(mean=np.zeros(2), cov=100.0 * np.identity(2))
    model = utils.elliptic()
    rng = np.random.RandomState(0)
    cloud = np.vstack([-2.65 + 0.07 * rng.standard_normal(50), 104.5 + 0.25 * rng.standard_normal(50)])
    for M in (65536, 1024):
        enka = calibrate.enka(2, 2, M)
        enka.Ustar = cloud[:, rng.randint(0, 50, M)]
        mc = sample.MCMC()
        mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, Y, "device", "float64"
        call = lambda n, **kw: mc.model_mh(model, n, prior, enka, Gamma, delta=1.0, chains=M, start="ensemble",     # noqa: E731
                                           fused=True, **kw)
        res = {mode: timed(mc, call, args.steps, mode, 1, args.mem) for mode in MODES}
        res["rhat"] = [round(float(v), 4) for v in mc.summary["rhat"]]
        res["ess"] = [round(float(v), 1) for v in mc.summary["ess"]]
        out["elliptic/%d" % M] = res
        out["clock_ghz"] = round(mc._mh_eng.calibrate_mfma()[1], 3)
        mc._mh_eng.close()


def lineal(args, out):
    from scipy import stats
    from ces_amd import calibrate, sample, utils
    p = n = 256
    M = 65536
    rng = np.random.default_rng(0)
    A = rng.standard_normal((n, p)) / np.sqrt(p)
    gam = np.full(n, 0.1)
    y = A @ (0.5 * rng.standard_normal(p)) + np.sqrt(gam) * rng.standard_normal(n)
    prior = stats.multivariate_normal(mean=np.zeros(p), cov=np.eye(p))
    model = utils.lineal(A)
    enka = calibrate.enka(p, n, 64)
    enka.Ustar = 0.3 * rng.standard_normal((p, 64))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, y, "device", "float32"
    call = lambda k, **kw: mc.model_mh(model, k, prior, enka, np.diag(gam), delta=float(np.sqrt(2 * 0.15 / n)),       # noqa: E731
                                       enka_scaling=False, chains=M, **kw)
    for stride, steps in zip((1, 10), args.lineal_steps):
        out["lineal/stride%d" % stride] = dict({mode: timed(mc, call, steps, mode, stride, args.mem) for mode in MODES},
                                               steps=steps)
    out["clock_ghz"] = round(mc._mh_eng.calibrate_mfma()[1], 3)
    mc._mh_eng.close()


def kernels(args, out):
    """The stage's launches alone, per draw."""
    import torch
    from ces_amd import engine
    for name, p, M, dtype, kept, reps in (("elliptic", 2, 65536, "float64", args.steps, 3), ("lineal", 256, 65536, "float32", 1, 8)):
        eng = engine.Engine(p, p, M, dtype=dtype)
        t = torch.randn((kept, p, M), dtype=eng.torch_dtype, device=eng.device)
        N = kept * (reps + 1)
        eng.chain_summary_begin(N)
        eng.chain_summary_add(t)                               # the first add: also the row means
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            eng.chain_summary_add(t)
        b.record()
        torch.cuda.synchronize()
        add_us = a.elapsed_time(b) * 1e3 / (reps * kept)
        t0 = time.perf_counter()
        eng.chain_summary_read()
        out["kernels/%s" % name] = dict(p=p, chains=M, dtype=dtype, draws_per_add=kept, add_us_per_draw=round(add_us, 3),
                                        read_ms=round((time.perf_counter() - t0) * 1e3, 3))
        out["clock_ghz"] = round(eng.calibrate_mfma()[1], 3)
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", default=["elliptic", "lineal", "kernels"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--lineal-steps", type=int, nargs=2, default=[16, 40])
    ap.add_argument("--mem", action="store_true")
    args = ap.parse_args()
    out = {}
    for name, fn in (("elliptic", elliptic), ("lineal", lineal), ("kernels", kernels)):
        if name in args.only:
            fn(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
