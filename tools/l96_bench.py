#!/usr/bin/env python3
"""Price the Lorenz '96 forward map on the device (cesx_lorenz_apply) against the host's solve_ivp loop at shape L1.

    python tools/l96_bench.py [--J 1024] [--T 20] [--host 4] [--steps 3] [--warmup 1] [--dtype float64]

L1 = lorenz96() defaults (36 slow x 10 fast), set_solver(T=20, dt=0.1), t = linspace(0, T, 10 T + 1), J = 1024, parameters
N((1, 10, log 10, 10), (.1, 1, .1, 1)), every particle started from generate_initial() (seed 1) times 1 + 0.05 N(0, 1).
Prints one JSON line:
    device_ms             one evaluation of the ensemble, HIP events around `steps` back-to-back launches
    accepted, attempted   steps per particle: min / median / max
    host_s_per_particle   model.solve + model.statistics on the first `host` particles, on this box
    speedup               host_s_per_particle * J / device time
    flagged               particles with a nonzero status
    clock_ghz             the in-kernel clock class of the box (cesx_calibrate_mfma)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--J", type=int, default=1024)
    ap.add_argument("--T", type=float, default=20.0)
    ap.add_argument("--host", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="float64")
    args = ap.parse_args()
    import torch
    from ces_amd import engine, models
    J = args.J
    mdl = models.lorenz96()
    mdl.set_solver(T=args.T, dt=0.1, device=True)
    t = np.linspace(0.0, args.T, int(round(10 * args.T)) + 1)
    rng = np.random.RandomState(0)
    Uh = (np.array([1.0, 10.0, np.log(10.0), 10.0])[:, None]
          + np.array([0.1, 1.0, 0.1, 1.0])[:, None] * rng.standard_normal((4, J))).astype(args.dtype).astype(np.float64)
    np.random.seed(1)
    w0 = mdl.generate_initial()
    Wh = w0[:, None] * (1.0 + 0.05 * rng.standard_normal((w0.size, J)))
    eng = engine.Engine(4, 5 * mdl.n_slow, J, dtype=args.dtype)
    U = eng.to_device(Uh, 4, "U")
    W = torch.as_tensor(Wh, device=eng.device)
    mdl.ensure_installed(eng, t)
    G, W_out = eng.empty(5 * mdl.n_slow), torch.empty_like(W)
    for _ in range(args.warmup):
        eng.l96_apply(U, W, out=G, W_out=W_out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.steps):
        _, _, info = eng.l96_apply(U, W, out=G, W_out=W_out)
    b.record()
    b.synchronize()
    device_ms = a.elapsed_time(b) / args.steps
    info = info.cpu().numpy()
    nh = min(args.host, J)
    t0 = time.perf_counter()
    Gh = np.stack([mdl.statistics(mdl.solve(Wh[:, j], t, args=tuple(Uh[:, j]))) for j in range(nh)], axis=1)
    host_s = (time.perf_counter() - t0) / max(nh, 1)
    _, ghz = eng.calibrate_mfma()

    def mmm(v):
        return [int(v.min()), float(np.median(v)), int(v.max())]
    print(json.dumps(dict(shape=dict(J=J, n_slow=mdl.n_slow, n_fast=mdl.n_fast, T=args.T, dt=0.1, samples=int(t.size),
                                     dtype=args.dtype),
                          device_ms=round(device_ms, 3), accepted=mmm(info[1]), attempted=mmm(info[2]),
                          host_particles=nh, host_s_per_particle=round(host_s, 3),
                          speedup=round(host_s * J / (device_ms * 1e-3), 1), flagged=int(np.count_nonzero(info[0])),
                          host_stat_scale=float(np.abs(Gh).max()) if nh else None, clock_ghz=round(ghz, 3))))


if __name__ == "__main__":
    main()
