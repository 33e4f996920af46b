#!/usr/bin/env python3
"""Time the training of the GP emulators on the device (cesx_gpfit_*) against the host path, on the same box.

    python tools/gpfit_bench.py [--jt 512 1024] [--n 32] [--p 8] [--maxiter 1000] [--host-train-gps 32] [--no-prof]

Shape T1 (the emulator of E1 in NOTEBOOK.md): 32 GPs, J_t = 512, p = 8, Matern-3/2 ARD, Linear mean; and J_t = 1024.
Per J_t, every step a child process of its own under its own time limit (the parent never opens the GPU; a step that
fails ends the run):
    eval        one batched gpfit_eval of all GPs: median of 20 after 5 warm-ups
    prof        the same step under ``rocprofv3 --kernel-trace --stats``: the split per kernel (a run of its own)
    train       train_gps(device=True) wall time (engine set-up, every lockstep round, the final factors)
    host-eval   GPR.log_marginal_likelihood_and_grad() of the same GPs at the same parameters, one after the other
    host-train  train_gps() on the host for the first --host-train-gps outputs (all of them by default)
Prints one JSON line per step and a last line with everything.  The evaluation's flop count for the fp64-MFMA fraction:
per GP the sums of the factorisation, of its triangular inverse and of the lower triangle of K^{-1} = W W^T on the matrix
pipe, J^3 / 6 multiply-adds each = J^3 flops in all (the 16 x 16 x 16 block products the kernels issue come to 1.001 J^3 at
J_t = 512; the diagonal blocks every workgroup repeats are not counted).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_MFMA = 78.2e12


class Enka(object):
    pass


def problem(n, Jt, p):
    rng = np.random.default_rng(0)
    U = rng.standard_normal((p, Jt))
    W = rng.standard_normal((p, n))
    G = (np.sin(U.T @ W) + 0.2 * (U.T ** 2) @ np.abs(W) + 0.05 * rng.standard_normal((Jt, n))).T
    enka = Enka()
    enka.p, enka.n_obs, enka.Ustar, enka.Gstar = p, n, U, G
    theta = np.hstack([0.5 + rng.random((n, 1)), (1.5 + rng.random((n, p))) * np.sqrt(p), np.full((n, 1), 1e-4),
                       0.1 * rng.standard_normal((n, p + 1))])
    return enka, theta


def step_eval(a):
    from ces_amd import engine
    enka, theta = problem(a.n, a.jt, a.p)
    eng = engine.Engine(a.p, 1, 1, dtype="float64")
    eng.gpfit_set(enka.Ustar.T, enka.Gstar, 2, True, "linear")
    idx = np.arange(a.n, dtype=np.int32)
    ts = []
    for it in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        lml, grad, status = eng.gpfit_eval(idx, theta)
        ts.append(time.perf_counter() - t0)
    assert np.all(status == 0) and np.all(np.isfinite(grad))
    ms = float(np.median(ts[a.warmup:]) * 1e3)
    flops = 1.0 * a.n * float(a.jt) ** 3
    return dict(step="eval", jt=a.jt, n=a.n, p=a.p, eval_ms=ms, eval_ms_min=float(min(ts[a.warmup:]) * 1e3),
                mfma_flops=flops, frac_f64_mfma_peak_of_wall=flops / (ms * 1e-3) / PEAK_F64_MFMA, lml0=float(lml[0]))


def step_train(a):
    from ces_amd import emulate as em
    enka, _ = problem(a.n, a.jt, a.p)
    t0 = time.perf_counter()
    em.train_gps(enka, kernel="Matern32", mean_function="Linear", maxiter=a.maxiter, device=True)
    wall = time.perf_counter() - t0
    nfev = [m.optimizer.result.nfev for m in enka.gpmodels]
    return dict(step="train", jt=a.jt, n=a.n, p=a.p, maxiter=a.maxiter, train_s=wall, rounds=int(max(nfev)), nfev_sum=int(sum(nfev)),
                success=int(sum(bool(m.optimizer.result.success) for m in enka.gpmodels)))


def step_host_eval(a):
    from ces_amd import emulate as em
    enka, theta = problem(a.n, a.jt, a.p)
    X = enka.Ustar.T
    models = []
    for i in range(a.n):
        m = em.GPR(X, enka.Gstar[i][:, None], em.Matern32(input_dim=a.p, ARD=True), mean_function=em.Linear(np.ones((a.p, 1))))
        m._set(theta[i][:a.p + 2], theta[i][a.p + 2:])
        models.append(m)
    models[0].log_marginal_likelihood_and_grad()                                  # (warm-up: BLAS threads, page faults)
    t0 = time.perf_counter()
    out = [m.log_marginal_likelihood_and_grad() for m in models]
    wall = time.perf_counter() - t0
    return dict(step="host-eval", jt=a.jt, n=a.n, p=a.p, host_eval_all_ms=wall * 1e3, host_eval_one_ms=wall * 1e3 / a.n,
                lml0=float(out[0][0]), cpus=len(os.sched_getaffinity(0)), omp=os.environ.get("OMP_NUM_THREADS"))


def step_host_train(a):
    from ces_amd import emulate as em
    enka, _ = problem(a.n, a.jt, a.p)
    k = min(a.n, a.host_train_gps)
    enka.n_obs = k
    t0 = time.perf_counter()
    em.train_gps(enka, kernel="Matern32", mean_function="Linear", maxiter=a.maxiter)
    wall = time.perf_counter() - t0
    return dict(step="host-train", jt=a.jt, gps=k, of=a.n, p=a.p, maxiter=a.maxiter, host_train_s=wall, host_train_s_per_gp=wall / k)


STEPS = {"eval": step_eval, "train": step_train, "host-eval": step_host_eval, "host-train": step_host_train}


def kernel_split(d):
    """{kernel: (calls, total us)} from rocprofv3's *_kernel_stats.csv under d"""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return None
    out = {}
    for r in csv.DictReader(open(files[-1])):
        name = r.get("Name", "")
        if "gpfit_" in name:
            name = name[name.index("gpfit_"):].split("(")[0]
            out[name] = dict(calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3)
    return out


def child(step, a, limit, prof_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--jt", str(a.jt), "--n", str(a.n), "--p", str(a.p),
           "--maxiter", str(a.maxiter), "--steps", str(a.steps), "--warmup", str(a.warmup), "--host-train-gps", str(a.host_train_gps)]
    if prof_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "--"] + cmd
    proc = subprocess.Popen(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    t0 = time.perf_counter()
    while True:                                   # (a sign of life per minute: the host steps run for minutes without output)
        try:
            out, err = proc.communicate(timeout=60)
            break
        except subprocess.TimeoutExpired:
            sys.stderr.write("gpfit_bench: step %s (J_t = %d) running, %.0f s\n" % (step, a.jt, time.perf_counter() - t0))
            sys.stderr.flush()
    res = subprocess.CompletedProcess(cmd, proc.returncode, out, err)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit("gpfit_bench: step %s (J_t = %d) ended with status %d; nothing more is started" % (step, a.jt, res.returncode))
    lines = [ln for ln in res.stdout.split("\n") if ln.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jt", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=1000)
    ap.add_argument("--host-train-gps", type=int, default=32)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--skip", nargs="*", default=[], help="steps to leave out (eval prof train host-eval host-train)")
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--step", choices=sorted(STEPS))
    a = ap.parse_args()
    if a.step:
        a.jt = a.jt[0]
        print(json.dumps(STEPS[a.step](a)), flush=True)
        return
    allres = []
    for jt in a.jt:
        a.jt = jt
        for step in ("eval", "prof", "train", "host-eval", "host-train"):
            if step in a.skip or (step == "prof" and a.no_prof):
                continue
            if step == "prof":
                d = tempfile.mkdtemp(prefix="gpfit_prof_")
                try:
                    r = child("eval", a, a.limit, prof_dir=d)
                    split = kernel_split(d)
                finally:
                    shutil.rmtree(d, ignore_errors=True)
                evals = a.steps + a.warmup
                r = dict(step="prof", jt=jt, evals=evals, kernels=split)
                if split:
                    tot = sum(v["total_us"] for v in split.values()) / evals
                    mm = sum(v["total_us"] for k, v in split.items() if k in ("gpfit_chol_kernel", "gpfit_kinv_kernel")) / evals
                    r.update(kernel_us_per_eval=tot, mfma_kernels_us_per_eval=mm,
                             frac_f64_mfma_peak_in_mfma_kernels=1.0 * a.n * float(jt) ** 3 / (mm * 1e-6) / PEAK_F64_MFMA)
            else:
                r = child(step, a, a.limit)
            print(json.dumps(r), flush=True)
            allres.append(r)
    print(json.dumps(dict(tool="gpfit_bench", results=allres)), flush=True)


if __name__ == "__main__":
    main()
