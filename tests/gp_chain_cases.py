"""Cases shared by the tests of the fused chain kernel of MCMC.gp_mh (test_gp_chain_host.py, test_gpu_gp_chain.py): the small
emulators and problems, a pairwise selection of shapes and modes, and an fp64 numpy restatement of the chains under the
device noise (oracle/philox.py) that reports how far every Metropolis decision sits from its threshold."""
import os
import sys

import numpy as np
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from gp_cases import random_gps  # noqa: E402
from oracle import stage_ref as sr  # noqa: E402

FAMILIES = ["RBF", "Matern12", "Matern32", "Matern52"]
K_STEPS = 7
DELTA, BETA = 0.3, 0.3
SEED = 77                                   # mc.seed of the device noise

# The smallest shapes at which something can go wrong: M around the tile of 32 chains and a second tile; J_t around the pad
# to 16 and a second block row of L^{-1}; p = 5 spans two Philox row quads; n = 1 and several GPs in turn.  The cycle lengths
# 5, 4 and 3 are coprime: twenty cases hold every (M, J_t) pair, every (M, p) and every (J_t, p) pair.
_MS, _JTS, _PS, _NS = (1, 31, 32, 33, 65), (15, 16, 17, 33), (1, 2, 5), (1, 4)
_MODES = ("gamma", "gamma_dense", "var", "gamma_var")
_PRIORS = ("rw_dense", "pcn", "rw_diag")


def cases():
    out = []
    for i in range(20):
        out.append(dict(M=_MS[i % 5], Jt=_JTS[i % 4], p=_PS[i % 3], n=_NS[(i // 3) % 2], family=FAMILIES[(i // 2) % 4],
                        nugget=bool((i // 5) % 2), mode=_MODES[(i + i // 4) % 4], prior=_PRIORS[(i + i // 3) % 3], seed=100 + i))
    return out


def case_id(c):
    return "M%d-Jt%d-p%d-n%d-%s-%s-%s-%s" % (c["M"], c["Jt"], c["p"], c["n"], c["family"], "nug" if c["nugget"] else "nonug",
                                             c["mode"], c["prior"])


def problem(c):
    """(enka, y, prior, kw): the emulator, the data, the prior and the kwargs of ``gp_mh`` for case ``c``."""
    rng = np.random.default_rng(c["seed"])
    p, n = c["p"], c["n"]
    enka = random_gps(rng, p, n, c["Jt"], c["family"], scaled=bool(c["seed"] % 2) and p > 1)
    y = enka.Gstar.mean(axis=1) + 0.1 * rng.standard_normal(n)
    B = rng.standard_normal((n, n))
    gam = 0.05 + 0.05 * rng.random(n)
    kw = dict(nugget=c["nugget"], delta=DELTA, enka_scaling=p > 1)
    if c["mode"] == "gamma":
        kw["Gamma"] = np.diag(gam)
    elif c["mode"] == "gamma_dense":
        kw["Gamma"] = np.diag(gam) + 0.02 * B @ B.T
    elif c["mode"] == "gamma_var":
        kw["Gamma"], kw["noise_compounded"] = np.diag(gam), True
    mu = enka.Ustar.mean(axis=1) + 0.1 * rng.standard_normal(p)
    C = rng.standard_normal((p, p))
    cov = np.diag(0.5 + rng.random(p))
    if c["prior"] != "rw_diag":
        cov = cov + 0.3 * C @ C.T
    if c["prior"] == "pcn":
        kw["update"], kw["beta"] = "pCN", BETA
    return enka, y, stats.multivariate_normal(mean=mu, cov=cov), kw


def scales_of(enka, kw):
    p = enka.p
    return kw["delta"] * np.linalg.cholesky(np.cov(enka.Ustar)) if kw["enka_scaling"] else kw["delta"] * np.eye(p)


def np_predict(enka, gps, X, nugget=True):
    """(mean, var) of the GPs at the rows of X, fp64 numpy (tests/test_gpu_gp.py: np_predict, without its bars)."""
    from ces_amd import emulate as em
    img = em.device_image(enka, gps)
    means, vars_ = [], []
    for i, m in enumerate(gps):
        Z = (img["A"][i] @ (X.T - img["c"][:, None])).T
        d = Z[:, None, :] - img["Z"][i][None, :, :]
        Ks = m.kern.variance * m.kern.f(np.sqrt((d * d).sum(-1)))
        means.append(Ks @ img["alpha"][i] + Z @ img["mw"][i] + img["par"][i, 2])
        W = img["Li"][i] @ Ks.T
        vars_.append(m.kern.variance - (W * W).sum(0) + (m.likelihood.variance if nugget else 0.0))
    return np.array(means), np.array(vars_)


def np_phi(enka, y, prior, kw, U):
    """(phi, sum of the absolute values of its terms) per column of U, fp64 numpy."""
    m, v = np_predict(enka, enka.gpmodels, U.T, kw.get("nugget", True))
    d = m - np.asarray(y)[:, None]
    Gamma = kw.get("Gamma", None)
    with np.errstate(all="ignore"):
        if Gamma is None or kw.get("noise_compounded", False):
            S = v + (np.diag(Gamma)[:, None] if Gamma is not None else 0.0)
            s, mag = (d * d / S + np.log(S)).sum(0), (d * d / np.abs(S) + np.abs(np.log(S))).sum(0)
        else:
            Gi = np.linalg.inv(Gamma)
            s = np.einsum("ij,ik,kj->j", d, Gi, d)
            mag = np.einsum("ij,ik,kj->j", np.abs(d), np.abs(Gi), np.abs(d))
        e = U - np.asarray(prior.mean).reshape(-1, 1)
        Si = np.linalg.inv(np.asarray(prior.cov).reshape(len(e), len(e)))
        s = s + np.einsum("ij,ik,kj->j", e, Si, e)
        mag = mag + np.einsum("ij,ik,kj->j", np.abs(e), np.abs(Si), np.abs(e))
    return 0.5 * s, 0.5 * mag


def np_chains(c, steps, first_step=0, U0=None, seed=SEED):
    """The chains of case ``c`` under the device noise of steps first_step .. first_step + steps - 1, fp64 numpy: (U, accept
    counters, the smallest |log u - (phi(U) - phi(P))| over all decisions, phi of the final states and its magnitude)."""
    enka, y, prior, kw = problem(c)
    p, M = enka.p, c["M"]
    S = scales_of(enka, kw)
    U = np.repeat(enka.Ustar.mean(axis=1).reshape(p, 1), M, axis=1) if U0 is None else U0.copy()
    a_, b_ = (np.sqrt(1 - BETA ** 2), np.sqrt(BETA)) if kw.get("update") == "pCN" else (1.0, 1.0)
    ph, _ = np_phi(enka, y, prior, kw, U)
    acc, margin = np.zeros(M, dtype=np.int64), np.inf
    for k in range(first_step, first_step + steps):
        xi = sr.mh_noise(p, M, seed, k, 0, np.float64)
        lu = sr.log_uniform(M, seed, k, 0)
        P = a_ * U + b_ * S @ xi
        pp, _ = np_phi(enka, y, prior, kw, P)
        with np.errstate(invalid="ignore"):
            gap = lu - (ph - pp)
            t = gap < 0
        margin = min(margin, float(np.nanmin(np.abs(gap))) if np.any(np.isfinite(gap)) else np.inf)
        U[:, t], ph[t] = P[:, t], pp[t]
        acc += t
    return U, acc, margin, np_phi(enka, y, prior, kw, U)
