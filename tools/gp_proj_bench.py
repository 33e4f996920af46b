#!/usr/bin/env python3
"""Time the projected per-chain likelihood of gp_mh(chains=, pca_tools=, sigma_form='projected') (cesx_gp_proj_set,
gp_score_proj_kernel) beside the dense one (cesx_gp_dense_set, gp_score_dense_kernel).

    python tools/gp_proj_bench.py [--p 4] [--jt 256] [--reps 20] [--warmup 3] [--rounds 2] [--min-ms 200]

For (n, k, M) = (50, 8, 65 536) and (128, 16, 8 192): the score launch of both modes (gp_accept in mode 'dense' and in mode
'proj') on one engine, the same states and the same GP rows, in one process, the two modes alternating ``rounds`` times;
each timing is HIP events around ``reps`` launches -- or as many more as fill a window of ``min-ms`` milliseconds (the
projected launch takes tens of microseconds: twenty of them measure the clock) -- the smallest of the rounds is reported
beside all of them.  For
(180, 16, 65 536), past the dense mode's n_obs <= 128: the projected mode alone.  Prints one JSON line per shape with
``proj_not_slower`` where both ran; the shader clock comes from the engine's in-kernel clock calibration
(cesx_calibrate_mfma) before and after.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gp_dense_bench import events_ms, problem  # noqa: E402


def timed_ms(torch, fn, args):
    """(ms per launch, launches in the timed window)"""
    ms = events_ms(torch, fn, args.reps, args.warmup)
    reps = args.reps
    if ms * reps < args.min_ms:
        reps = int(np.ceil(args.min_ms / ms))
        ms = events_ms(torch, fn, reps, 0)
    return ms, reps


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
    modes = ["proj"]
    eng.gp_proj_set(*em.project_sigma(Gamma, VD_k, mG, y_obs), True)
    if n <= engine.GP_DENSE_NMAX:
        eng.gp_dense_set(VD_k, mG, True)
        modes = ["dense", "proj"]
    X = eng.to_device(0.5 * rng.standard_normal((p, M)), p).clone()
    P = eng.empty(p)
    mean = torch.empty((k, M), dtype=torch.float64, device=eng.device)
    var = torch.empty_like(mean)
    eng.gp_predict(X, out=(mean, var))
    eng.gp_start("proj", X, mean, var)
    eng.mh_propose(0, X, out=P)
    eng.gp_predict(P, out=(mean, var))
    ms, launches = {m: [] for m in modes}, {}
    for _ in range(args.rounds):
        for m in modes:
            t, launches[m] = timed_ms(torch, lambda s: eng.gp_accept(m, s, X, P, mean, var), args)
            ms[m].append(t)
    _, ghz1 = eng.calibrate_mfma()
    out = dict(shape=dict(n=n, k=k, chains=M, p=p, J_t=args.jt), shader_ghz=[ghz0, ghz1])
    for m in modes:
        out["ms_score_" + m] = min(ms[m])
        out["ms_score_%s_rounds" % m] = ms[m]
        out["launches_%s" % m] = launches[m]
        out["us_score_%s_per_chain" % m] = 1e3 * min(ms[m]) / M
    if "dense" in ms:
        out["proj_not_slower"] = bool(min(ms["proj"]) <= min(ms["dense"]))
        out["dense_over_proj"] = min(ms["dense"]) / min(ms["proj"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--jt", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=200.0)
    args = ap.parse_args()
    for n, k, M in ((50, 8, 65536), (128, 16, 8192), (180, 16, 65536)):
        print(json.dumps(device_times(args, n, k, M, np.random.default_rng([n, k]))), flush=True)


if __name__ == "__main__":
    main()
