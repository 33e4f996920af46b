#!/usr/bin/env python3
"""Price the Lorenz '63 forward map on the device (cesx_lorenz_three_apply) against the host's per-particle solve at the
shape of the reference's notebook (examples/notebooks/lorenz63.ipynb).

    python tools/l63_bench.py [--J 1024 65536] [--host 4] [--steps 5] [--warmup 2] [--dtype float64]

Shape: lorenz63_log(l_window=10, freq=100), t = arange(0, 40, 0.01) plus one sample (4001 samples: four whole windows of
1000 after the first), set_solver() defaults (RK45, rtol 1e-3, atol 1e-6, no max_step), parameters
(log 28, log 8/3) + 0.1 N(0, 1), every particle started from one attractor state times 1 + 0.05 N(0, 1).
Prints one JSON line:
    device_ms             per J: one evaluation of the ensemble, HIP events around `steps` back-to-back launches
    accepted, attempted   per J: steps per particle, min / median / max
    host_ivp_s, host_odeint_s   model.solve + model.statistics per particle (solve_ivp after set_solver / odeint, the
                          reference's integrator), mean over the first `host` particles, on this box
    speedup_ivp           per J: host_ivp_s * J / device time
    flagged               per J: particles with a nonzero status
    clock_ghz             the in-kernel clock class of the box (cesx_calibrate_mfma)
    bar                   one evaluation of 1024 particles takes less time than 1024 host solve calls on this box; the
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--J", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--host", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="float64")
    args = ap.parse_args()
    import torch
    from ces_amd import engine, models
    t = 0.01 * np.arange(4001)
    mdl = models.lorenz63_log(l_window=10, freq=100)
    mdl.set_solver(device=True)
    ref = models.lorenz63_log(l_window=10, freq=100)               # no set_solver: odeint, as the reference integrates
    w0 = np.array([-5.6, -9.3, 15.2])
    device_ms, accepted, attempted, flagged, speedup = {}, {}, {}, {}, {}

    def mmm(v):
        return [int(v.min()), float(np.median(v)), int(v.max())]
    Uh = Wh = None
    ghz = 0.0
    for J in args.J:
        rng = np.random.RandomState(0)
        Uh = (np.log([28.0, 8.0 / 3])[:, None] + 0.1 * rng.standard_normal((2, J))).astype(args.dtype).astype(np.float64)
        Wh = w0[:, None] * (1.0 + 0.05 * rng.standard_normal((3, J)))
        eng = engine.Engine(2, 9, J, dtype=args.dtype)
        U = eng.to_device(Uh, 2, "U")
        W = torch.as_tensor(Wh, device=eng.device)
        mdl.ensure_installed(eng, t)
        G, W_out = eng.empty(9), torch.empty_like(W)
        for _ in range(args.warmup):
            eng.l63_apply(U, W, out=G, W_out=W_out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            _, _, info = eng.l63_apply(U, W, out=G, W_out=W_out)
        b.record()
        b.synchronize()
        device_ms[J] = a.elapsed_time(b) / args.steps
        info = info.cpu().numpy()
        accepted[J], attempted[J], flagged[J] = mmm(info[1]), mmm(info[2]), int(np.count_nonzero(info[0]))
        _, ghz = eng.calibrate_mfma()
    nh = max(1, min(args.host, min(args.J)))
    host = {}
    for key, m in (("ivp", mdl), ("odeint", ref)):
        t0 = time.perf_counter()
        for j in range(nh):
            m.statistics(m.solve(Wh[:, j], t, args=tuple(Uh[:, j])))
        host[key] = (time.perf_counter() - t0) / nh
    for J in args.J:
        speedup[J] = round(host["ivp"] * J / (device_ms[J] * 1e-3), 1)
    bar = None
    if 1024 in device_ms:
        bar = bool(device_ms[1024] * 1e-3 < 1024 * min(host.values()))
    print(json.dumps(dict(shape=dict(J=args.J, samples=int(t.size), window=1000, dtype=args.dtype),
                          device_ms={str(k): round(v, 3) for k, v in device_ms.items()},
                          accepted={str(k): v for k, v in accepted.items()}, attempted={str(k): v for k, v in attempted.items()},
                          host_particles=nh, host_ivp_s=round(host["ivp"], 4), host_odeint_s=round(host["odeint"], 4),
                          speedup_ivp={str(k): v for k, v in speedup.items()},
                          flagged={str(k): v for k, v in flagged.items()}, clock_ghz=round(ghz, 3), bar=bar)))
    return 0 if bar in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
