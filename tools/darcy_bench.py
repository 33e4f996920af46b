#!/usr/bin/env python3
"""Price the Darcy forward map on the device (cesx_darcy_apply) against the host map at benchmark shape C4.

    python tools/darcy_bench.py [--J 8192] [--p 64] [--n 50] [--K 16] [--scale 10] [--host 256] [--steps 20] [--warmup 3]
                                [--dtype float32] [--solver resident|streamed] [--max-workgroups 0]

J = 8 192 particles, model_trunc(p = 64), 50 observations, Nmesh = 16, xi = scale N(0, I) (the example's U0 = 10 N(0, 1)).
--solver streamed installs the map for kernels_darcy_stream.hip (Nmesh up to 64; --max-workgroups bounds its grid, 0 = automatic).
Prints one JSON line:
    device_ms             one evaluation of the ensemble, HIP events around `steps` back-to-back cesx_darcy_apply launches
    hook_ms               the same through model.forward_device (adds the status read, which synchronises), wall clock
    host_s_scaled         the host's model(k) loop on the first `host` particles, scaled to J
    speedup               host_s_scaled / device time
    parity_worst_rel      max_j max|g_dev - g_host| / max|g_host| over the host-evaluated particles whose status is 0
                          (context, not a bound)
    flagged               particles with a nonzero status word (singular or not finite; their outputs are NaN)
    workspace_mb, grid    streamed: the HBM workspace of the installed map and the workgroups it launches
    clock_ghz, mfma_tflops  the in-kernel clock class of the box (cesx_calibrate_mfma)
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
    ap.add_argument("--J", type=int, default=8192)
    ap.add_argument("--p", type=int, default=64)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--scale", type=float, default=10.0)
    ap.add_argument("--host", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--solver", default="resident", choices=["resident", "streamed"])
    ap.add_argument("--max-workgroups", type=int, default=0)
    args = ap.parse_args()
    import torch
    from ces_amd import darcy, engine
    J, p, n, K = args.J, args.p, args.n, args.K
    rng = np.random.default_rng(0)
    mdl = darcy.model_trunc(Nmesh=float(K), p=p) if p < K * K else darcy.model(Nmesh=float(K))
    mdl.obs_index = rng.choice(K * K, n, replace=False)
    mdl.set_device_solver(args.solver)
    mdl.device_max_workgroups = args.max_workgroups
    eng = engine.Engine(p, n, J, dtype=args.dtype)
    Uh = (args.scale * rng.standard_normal((p, J))).astype(args.dtype).astype(np.float64)
    U = eng.to_device(Uh, p, "U")
    G = eng.empty(n)
    status = torch.zeros(J, dtype=torch.int32, device=eng.device)
    mdl.forward_device(eng, U, out=G)                       # installs the map

    def launch():
        eng._check(eng.lib.cesx_darcy_apply(eng._h, U.data_ptr(), G.data_ptr(), status.data_ptr(), eng._stream()))
    for _ in range(args.warmup):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.steps):
        launch()
    b.record()
    b.synchronize()
    device_ms = a.elapsed_time(b) / args.steps
    t0 = time.perf_counter()
    for _ in range(args.steps):
        mdl.forward_device(eng, U, out=G)
    torch.cuda.synchronize()
    hook_ms = (time.perf_counter() - t0) / args.steps * 1e3
    Gd = G.cpu().numpy().astype(np.float64)
    nh = min(args.host, J)
    t0 = time.perf_counter()
    Gh = np.stack([mdl(Uh[:, j]) for j in range(nh)], axis=1)
    host_s = time.perf_counter() - t0
    ok = status.cpu().numpy()[:nh] == 0
    rel = np.max(np.abs(Gd[:, :nh] - Gh), axis=0)[ok] / np.max(np.abs(Gh), axis=0)[ok]
    tf, ghz = eng.calibrate_mfma()
    ws = eng.darcy_workspace_bytes()
    m = K - 2
    print(json.dumps(dict(shape=dict(J=J, p=p, n_obs=n, K=K, scale=args.scale, dtype=args.dtype), solver=args.solver,
                          workspace_mb=round(ws / 1e6, 1), grid=ws // (m * m * (2 * m + 1) * 8) if ws else J, device_ms=round(device_ms, 4),
                          hook_ms=round(hook_ms, 4), host_particles=nh, host_s=round(host_s, 3),
                          host_s_scaled=round(host_s / nh * J, 2), speedup=round(host_s / nh * J / (device_ms * 1e-3), 1),
                          parity_worst_rel=float(rel.max()) if rel.size else None, flagged=int(torch.count_nonzero(status)),
                          clock_ghz=round(ghz, 3), mfma_tflops=round(tf, 2))))


if __name__ == "__main__":
    main()
