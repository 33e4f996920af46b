"""Shared cases of model_mh / gp_mh(adapt=) (tests/test_adapt_host.py, tests/test_gpu_adapt.py): the vectorised fp64 numpy
restatement of pooled step-size adaptation, written from include/cesx.h (cesx_mh_adapt_*), not from ces_amd.sample, on the
problems, phi and g of tests/map_langevin_cases.py and tests/gp_langevin_cases.py.

With S the scale the sampler forms, g = S^T grad phi and e one multiplier shared by all M chains (e_1 = 1), adaptation step
t = 1 .. A is

    xi ~ N(0, I_p);  r = xi - (e / 2) g(U);  Q = U + e S r
    L - 1 times:  phi(Q), g(Q);  r = r - e g(Q);  Q = Q + e S r
    last:         phi(Q), g(Q);  r = r - (e / 2) g(Q)
    d = phi(U) - phi(Q) + |xi|^2 / 2 - |r|^2 / 2;  accept iff log u < d
    alpha_j = 1 if d >= 0, exp(d) if d < 0, 0 if d is NaN;   abar_t = mean_j alpha_j
    log e_{t+1} = log e_t + (gain / sqrt(t)) (abar_t - target)
    log ebar_t  = t^-kappa log e_{t+1} + (1 - t^-kappa) log ebar_{t-1},   log ebar_0 = 0

with the draws of ``hmc_cases._hmc_steps`` (per step the xi block, then the uniforms).  The result is ebar_A."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_langevin_cases as gc  # noqa: E402
import hmc_cases as hc  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402

ENTRY_POINTS = ("cesx_mh_adapt_set", "cesx_mh_adapt_read")
STEPS_MAX = 65536
TARGET = {"langevin": 0.574, "hmc": 0.651}
GAIN, KAPPA = 2.0, 0.75
CAP = 1e-9


def np_adapt(score, S, U0, A, L, target, gain=GAIN, kappa=KAPPA, rnd=lambda a: a, poison=None):
    """``A`` adaptation steps of the columns of U0 with ``score(U) -> (phi (M,), g (p, M))`` from the global RNG as it
    stands.  ``rnd`` rounds every position (an fp32 engine stores Q in fp32).  ``poison(t, l, phq, gq)`` may overwrite phi and g
    of step t at leapfrog l in place (a NaN column in G: the NaN contract).  Returns (states after every step (A, p, M),
    history (A, 2) of (e_t, abar_t), ebar_A, the per-chain alpha of every step (A, M))."""
    U = rnd(np.array(U0, dtype=np.float64))
    p, M = U.shape
    phi, g = score(U)
    log_e = log_ebar = 0.0
    states, hist, alphas = [], np.zeros((A, 2)), np.zeros((A, M))
    for t in range(1, A + 1):
        e = np.exp(log_e)
        xi = np.random.normal(0, 1, [p, M])
        logu = np.log(np.random.uniform(size=M))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            r = xi - (0.5 * e) * g
            Q = rnd(U + e * (S @ r))
            for l in range(1, L + 1):
                phq, gq = score(Q)
                if poison is not None:
                    poison(t, l, phq, gq)
                if l < L:
                    r = r - e * gq
                    r[:, ~np.isfinite(phq)] = np.nan
                    Q = rnd(Q + e * (S @ r))
                else:
                    r = r - (0.5 * e) * gq
            d = phi - phq + (0.5 * (xi * xi).sum(axis=0) - 0.5 * (r * r).sum(axis=0))
            alpha = np.where(d >= 0, 1.0, np.where(d < 0, np.exp(np.minimum(d, 0.0)), 0.0))
            ok = logu < d
        U = U.copy()
        U[:, ok], phi[ok], g[:, ok] = Q[:, ok], phq[ok], gq[:, ok]
        abar = alpha.sum() / M
        hist[t - 1] = e, abar
        alphas[t - 1] = alpha
        states.append(U.copy())
        log_e = log_e + gain / np.sqrt(float(t)) * (abar - target)
        w = float(t) ** -kappa
        log_ebar = w * log_e + (1.0 - w) * log_ebar
    return np.array(states), hist, float(np.exp(log_ebar)), alphas


def map_score(kind, S, problem=None):
    prob = mc_.problem(kind, None) if problem is None else problem
    return lambda U: lc.np_phi_g(prob, S, U)


def gp_score(enka, gps, y, prior, S, mode, Gamma, nugget=True):
    def score(U):
        m, v, dm, dv, _, _ = gc.np_predict_grad(enka, gps, U.T, nugget)
        ph, grad = gc.np_phi_grad(m, v, dm, dv, U, y, mode, Gamma, np.asarray(prior.mean), np.asarray(prior.cov))
        return ph, S.T @ grad.T
    return score


def np_accept_rate(score, S, U0, steps, L):
    """The acceptance of ``steps`` plain HMC steps (no adaptation) over all chains, from the global RNG as it stands."""
    _, acc = hc._hmc_steps(score, S, U0, steps, L)
    return acc.sum() / (steps * U0.shape[1])


def scales(kind, factor=1.0):
    """``lc.scales(kind)`` at ``factor`` times ``lc.DELTA[kind]``, formed as model_mh forms it: delta chol(cov)."""
    return (factor * lc.DELTA[kind]) * np.linalg.cholesky(np.cov(mc_.start_ensemble(kind, 130, np.random.default_rng(4))))


def differing(U, Ur, cap=CAP):
    """The chains whose state differs from the reference's by more than cap (1 + |U|): a bool (M,)."""
    return np.any(np.abs(U - Ur) > cap * (1 + np.abs(Ur)), axis=0)
