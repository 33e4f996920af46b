#!/usr/bin/env python3
"""Price ``autocorr=`` (cesx_chain_acf_*: the lagged sums of the kept states on the device) on top of ``summary=True`` at the
two shapes of tools/chain_summary_bench.py.

    python tools/chain_autocorr_bench.py [--only elliptic lineal kernels] [--steps 1000] [--lineal-steps 128] [--lags 31]

elliptic   ces_amd.utils.elliptic, fused, fp64, 65 536 chains, `steps` steps in one launch: the stage reads the launch's trace
           in place
lineal     ces_amd.utils.lineal at p = n_obs = 256, 65 536 chains, fp32, the step path: one draw per add, 64 of them packed
           into the stage's own block before the lag kernel runs
Each at ``chains`` = 1 024 (the default) and = M.  Per shape and C the sampler call runs with ``summary=True`` alone and with
``autocorr=dict(lags=L, chains=C)``, alternating, twice each after one untimed call of each (the engine, the allocations):
wall time per step of every timed call, and the stage's modelled HBM bytes per draw and followed (row, chain):
    in place   e + (2 LT + 3) x 16 / kept           (the draw once; c, S1, P and the ring read and written once per launch)
    packed     3 e + (2 LT + 3) x 16 / 64           (the draw read, written to the block and read again; the sums per 64 draws)
with e the bytes of a draw's element and LT = 8, 32 or 64 the ring's slots.
kernels    the stage's launches alone (device events around ``chain_acf_add``, per draw) at the same shapes and both C.
``summary_alone`` is also what to compare across two builds of the library: the existing path's cost with this stage idle.
Prints one JSON line.  Nothing of this enters bench.py's value.
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
M = 65536


def lt_of(L):
    return 8 if L <= 8 else (32 if L <= 32 else 64)


def modelled_bytes(esz, L, kept):
    state = (2 * lt_of(L) + 3) * 16
    return round(esz + state / kept, 2) if kept >= 64 else round(3 * esz + state / 64, 2)


def timed(mc, call, steps, kw):
    import torch
    mc.__dict__.pop("samples", None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(steps, **kw)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e6 / steps, 2)


def priced(mc, call, steps, L, esz, kept, have_autocorr):
    out = {}
    for C in (1024, M):
        kws = {"summary_alone": dict(summary=True)}
        if have_autocorr:
            kws["with_autocorr"] = dict(summary=True, autocorr=dict(lags=L, chains=C))
        for kw in kws.values():                               # untimed: the engine, the stage's buffers
            timed(mc, call, steps, kw)
        res = {k: [] for k in kws}
        for _ in range(2):                                    # alternating
            for k, kw in kws.items():
                res[k].append(timed(mc, call, steps, kw))
        row = {k + "_us_per_step": v for k, v in res.items()}
        row["modelled_bytes_per_draw"] = modelled_bytes(esz, L, kept)
        if have_autocorr:
            a = mc.autocorr
            row.update(ess=[round(float(v), 1) for v in a["ess"][:4]], tau=[round(float(v), 2) for v in a["tau"][:4]],
                       truncated=int(a["truncated"].sum()), old_ess=[round(float(v), 1) for v in mc.summary["ess"][:4]])
        out["chains=%d" % C] = row
        if not have_autocorr:
            break
    return out


def elliptic(args, out):
    from scipy import stats
    from ces_amd import calibrate, sample, utils
    Gamma = 0.1 ** 2 * np.identity(2)
    prior = stats.multivariate_normal(mean=np.zeros(2), cov=100.0 * np.identity(2))
    model = utils.elliptic()
    rng = np.random.RandomState(0)
    cloud = np.vstack([-2.65 + 0.07 * rng.standard_normal(50), 104.5 + 0.25 * rng.standard_normal(50)])
    enka = calibrate.enka(2, 2, M)
    enka.Ustar = cloud[:, rng.randint(0, 50, M)]
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise, mc.engine_dtype = True, Y, "device", "float64"
    call = lambda n, **kw: mc.model_mh(model, n, prior, enka, Gamma, delta=1.0, chains=M, start="ensemble", fused=True, **kw)   # noqa: E731
    out["elliptic"] = dict(priced(mc, call, args.steps, args.lags, 8, args.steps, hasattr(sample, "finalise_autocorr")),
                           steps=args.steps, launches=mc.fused_launches)
    mc._mh_eng.close()


def lineal(args, out):
    from scipy import stats
    from ces_amd import calibrate, sample, utils
    p = n = 256
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
    out["lineal"] = dict(priced(mc, call, args.lineal_steps, args.lags, 4, 1, hasattr(sample, "finalise_autocorr")),
                         steps=args.lineal_steps)
    mc._mh_eng.close()


def kernels(args, out):
    """The stage's launches alone, per draw."""
    import torch
    from ces_amd import engine
    L = args.lags
    for name, p, dtype, kept, reps in (("elliptic", 2, "float64", args.steps, 3), ("lineal", 256, "float32", 1, 128)):
        for C in (1024, M):
            eng = engine.Engine(p, p, M, dtype=dtype)
            t = torch.randn((kept, p, M), dtype=eng.torch_dtype, device=eng.device)
            eng.chain_acf_begin(kept * (reps + 64), L, C)
            for _ in range(64):                               # the first adds: also the allocations, and a first block
                eng.chain_acf_add(t)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                eng.chain_acf_add(t)
            b.record()
            torch.cuda.synchronize()
            add_us = a.elapsed_time(b) * 1e3 / (reps * kept)
            t0 = time.perf_counter()
            eng.chain_acf_read()
            esz = 4 if dtype == "float32" else 8
            per = modelled_bytes(esz, L, kept)
            out["kernels/%s/chains=%d" % (name, C)] = dict(
                p=p, dtype=dtype, draws_per_add=kept, add_us_per_draw=round(add_us, 3), read_ms=round((time.perf_counter() - t0) * 1e3, 3),
                modelled_bytes_per_draw=per, modelled_gb_per_s=round(per * p * C / add_us / 1e3, 1))
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", default=["elliptic", "lineal", "kernels"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--lineal-steps", type=int, default=128)
    ap.add_argument("--lags", type=int, default=31)
    args = ap.parse_args()
    out = {}
    for name, fn in (("elliptic", elliptic), ("lineal", lineal), ("kernels", kernels)):
        if name in args.only:
            fn(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
