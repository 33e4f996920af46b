"""Shared cases of model_mh / gp_mh(update='hmc') (tests/test_hmc_host.py, tests/test_gpu_hmc.py), built on
tests/map_langevin_cases.py and tests/gp_langevin_cases.py: their problems, DELTA, scales, phi and g, and the vectorised fp64
numpy chains of the leapfrog step, written from the step of include/cesx.h (cesx_mh_hmc_*), not from ces_amd.sample:

    xi ~ N(0, I_p);  r = xi - g(U) / 2;  Q = U
    l = 1 .. L:  Q = Q + S r;  phi(Q), g(Q);  r = r - g(Q)  (l < L)  or  r = r - g(Q) / 2  (l = L)
    log u < phi(U) + |xi|^2 / 2 - phi(Q) - |r|^2 / 2  ->  U := Q, phi := phi(Q), g := g(Q)

with the draw order of ``np_chains_mala`` (per step the xi block, then the uniforms) and ONE draw of each per step whatever
L is.  A non-finite phi, g, r or Q anywhere in a trajectory rejects."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_langevin_cases as gc  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402

ENTRY_POINTS = ("cesx_mh_hmc_begin", "cesx_mh_hmc_leap", "cesx_mh_hmc_accept", "cesx_gp_hmc_leap", "cesx_gp_hmc_accept",
                "cesx_mh_hmc_run_map")
LEAPFROG_MAX, GRADS_MAX = 64, 4096


def _hmc_steps(score, S, U0, steps, L, kinetic=True, rnd=lambda a: a, keep=None):
    """``steps`` HMC steps of the columns of U0 with ``score(U) -> (phi (M,), g (p, M))`` from the global RNG as it stands.
    ``rnd`` rounds every position (an fp32 engine's step path stores Q in fp32).  Returns (U, accepted per chain)."""
    U = rnd(np.array(U0, dtype=np.float64))
    p, M = U.shape
    phi, g = score(U)
    acc = np.zeros(M, dtype=np.int64)
    for _ in range(steps):
        xi = np.random.normal(0, 1, [p, M])
        logu = np.log(np.random.uniform(size=M))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            r = xi - 0.5 * g
            Q = U
            bad = np.zeros(M, dtype=bool)
            for l in range(1, L + 1):
                Q = rnd(Q + S @ r)
                phq, gq = score(Q)
                r = r - gq if l < L else r - 0.5 * gq
                bad |= ~(np.isfinite(phq) & np.all(np.isfinite(gq), axis=0) & np.all(np.isfinite(r), axis=0)
                         & np.all(np.isfinite(Q), axis=0))
            kin = 0.5 * (xi * xi).sum(axis=0) - 0.5 * (r * r).sum(axis=0) if kinetic else 0.0
            ok = ~bad & (logu < phi - phq + kin)
        U = U.copy()
        U[:, ok], phi[ok], g[:, ok] = Q[:, ok], phq[ok], gq[:, ok]
        acc += ok
        if keep is not None:
            keep.append(U.copy())
    return U, acc


def np_chains_hmc(kind, S, U0, steps, L, seed, kinetic=True, problem=None):
    """``steps`` HMC steps of ``L`` leapfrogs of the M = U0.shape[1] chains on the problem of ``map_cases.problem(kind, None)``
    (or ``problem``) in vectorised fp64 numpy.  ``seed`` None: the global RNG as it stands.  ``kinetic=False`` drops both
    |.|^2 / 2 terms from the test (a wrong sampler: the failing control of the invariance test).  Returns (U, accepted per
    chain)."""
    prob = mc_.problem(kind, None) if problem is None else problem
    if seed is not None:
        np.random.seed(seed)
    with np.errstate(over="ignore", invalid="ignore"):
        return _hmc_steps(lambda U: lc.np_phi_g(prob, S, U), S, U0, steps, L, kinetic)


def np_chains_hmc_gp(enka, gps, y, prior, scales, U0, steps, L, mode, Gamma, nugget, seed, round32=False):
    """The GP counterpart, on ``gp_langevin_cases``' restatement of the emulator's rows and gradients (the draws of
    noise='numpy' under ``seed``; the global RNG is put back).  ``round32``: every position rounded to fp32, as an fp32
    engine stores it.  Returns (U, accept rate per chain)."""
    rng_state = np.random.get_state()
    np.random.seed(seed)

    def score(U):
        m, v, dm, dv, _, _ = gc.np_predict_grad(enka, gps, U.T, nugget)
        ph, grad = gc.np_phi_grad(m, v, dm, dv, U, y, mode, Gamma, np.asarray(prior.mean), np.asarray(prior.cov))
        return ph, scales.T @ grad.T

    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if round32 else (lambda a: a)
    U, acc = _hmc_steps(score, scales, U0, steps, L, rnd=rnd)
    np.random.set_state(rng_state)
    return U, acc / steps
