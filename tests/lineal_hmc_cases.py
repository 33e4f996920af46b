"""Shared cases of model_mh(update='hmc', adapt=) for the linear maps (tests/test_lineal_hmc_host.py,
tests/test_gpu_lineal_hmc.py), built on tests/lineal_langevin_cases.py -- its problems, DELTA, FORMS, scales, phi and g --
and on the vectorised fp64 numpy chains of tests/hmc_cases.py and tests/adapt_cases.py, which are written from the step of
include/cesx.h and not from ces_amd.sample.  With S the scale, g = S^T grad phi and e the multiplier (1 without adapt=):

    xi ~ N(0, I_p);  r = xi - (e / 2) g(U);  Q = U
    L times:  Q = Q + e S r;  G(Q), g(Q);  r = r - e g(Q), the last time r = r - (e / 2) g(Q)
    log u < phi(U) - phi(Q) + |xi|^2 / 2 - |r|^2 / 2  ->  U := Q, phi := phi(Q), g := g(Q)

One xi block and one uniform per step whatever L is."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapt_cases as ac  # noqa: E402
import hmc_cases as hc  # noqa: E402
import lineal_langevin_cases as lc  # noqa: E402

ENTRY_POINTS = ("cesx_mh_hmc_lineal_begin", "cesx_mh_hmc_lineal_leap", "cesx_mh_hmc_lineal_accept")
FACTORS = {"long": 8.0, "short": 1.0 / 16.0}               # delta = factor * lc.DELTA: a step 8 x too long, one 16 x too short


def model_of(prob, leapfrog=True):
    """The model of ``lineal_langevin_cases.model_of`` with the mark of ``enable_gradient(leapfrog=True)``."""
    mdl = lc.model_of(prob, gradient=False)
    return mdl.enable_gradient(leapfrog=True) if leapfrog else mdl.enable_gradient()


def sampler(prob, noise="device", dtype="float64", stride=1, seed=None):
    """(MCMC, enka, prior) on the problem's 130-particle start ensemble."""
    from scipy import stats
    from ces_amd import calibrate, sample
    enka = calibrate.enka(prob["p"], prob["n"], 130)
    enka.Ustar = prob["ens"]
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.engine_dtype, s.trace_stride = True, prob["y"], noise, dtype, stride
    if seed is not None:
        s.seed = seed
    return s, enka, stats.multivariate_normal(mean=prob["mu"], cov=prob["Sigma"])


def score_of(prob, S):
    return lambda U: lc.np_phi_g(prob, S, U)


def scales(prob, factor=1.0):
    """``lc.scales(prob)`` at ``factor`` times the problem's delta, formed as model_mh forms it: delta chol(cov)."""
    return (factor * prob["delta"]) * np.linalg.cholesky(np.cov(prob["ens"]).reshape(prob["p"], prob["p"]))


def np_chains(prob, S, U0, steps, L, seed, kinetic=True, keep=None):
    """``steps`` HMC steps of ``L`` leapfrogs of the columns of U0 (``hmc_cases._hmc_steps`` on this problem's score).  ``seed``
    None: the global RNG as it stands.  Returns (U, accepted per chain)."""
    if seed is not None:
        np.random.seed(seed)
    with np.errstate(over="ignore", invalid="ignore"):
        return hc._hmc_steps(score_of(prob, S), S, U0, steps, L, kinetic, keep=keep)


def np_positions(prob, S, U, xi, L, e=1.0):
    """The L positions of one trajectory from the states U (p, M) with the block xi, in fp64: [Q_1, .., Q_L]."""
    _, g = lc.np_phi_g(prob, S, U)
    r = xi - (0.5 * e) * g
    Q, out = U, []
    for l in range(1, L + 1):
        Q = Q + e * (S @ r)
        out.append(Q)
        if l < L:
            r = r - e * lc.np_phi_g(prob, S, Q)[1]
    return out
