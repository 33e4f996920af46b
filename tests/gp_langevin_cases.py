"""What the tests of gp_mh(update='langevin') share (test_gp_langevin_host.py, test_gpu_gp_langevin.py): the fp64 numpy
restatement of cesx_gp_predict_grad with its bars, and the vectorised restatement of the Langevin chains over the columns.
Written from the formulas of include/cesx.h, not from ces_amd.sample: the package's own numpy is checked against central
differences in test_gp_langevin_host.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import Enka  # noqa: E402


def np_predict_grad(enka, gps, X, nugget=True, beta_via="Li"):
    """mean, var (n, M), dmean, dvar (n, M, p) with respect to the unscaled X (M, p), and the bars' scales: the sums of
    absolute terms sum_t |alpha_t| |dk_t| + |w| and 2 sum_t |beta_t| |dk_t|, carried through |A|^T (n, M, p).
    beta_via: 'Li' forms beta = L^{-T} (L^{-1} k*) as the device does, 'K' solves (K + sn^2 I) beta = k*."""
    from ces_amd import emulate as em
    img = em.device_image(enka, gps)
    out = [[] for _ in range(6)]
    for i, m in enumerate(gps):
        A = img["A"][i]
        Z = (A @ (X.T - img["c"][:, None])).T                                    # (M, p)
        d = Z[:, None, :] - img["Z"][i][None, :, :]                              # (M, Jt, p): z - Z_t
        r = np.sqrt((d * d).sum(-1))
        Ks = m.kern.variance * m.kern.f(r)                                      # (M, Jt)
        a = img["alpha"][i]
        W = img["Li"][i] @ Ks.T
        if beta_via == "Li":
            beta = img["Li"][i].T @ W
        else:
            beta = np.linalg.solve(m.kern.K(m.X) + m.likelihood.variance * np.eye(len(m.X)), Ks.T)
        dk = (m.kern.variance * m.kern.dfr_over_r(r))[:, :, None] * d            # (M, Jt, p): dk_t / dz
        gzm = np.einsum("t,mtq->mq", a, dk) + img["mw"][i]
        gzv = -2.0 * np.einsum("tm,mtq->mq", beta, dk)
        out[0].append(Ks @ a + Z @ img["mw"][i] + img["par"][i, 2])
        out[1].append(m.kern.variance - (W * W).sum(0) + (m.likelihood.variance if nugget else 0.0))
        out[2].append(gzm @ A)                                                   # grad_x = A^T grad_z
        out[3].append(gzv @ A)
        out[4].append((np.einsum("t,mtq->mq", np.abs(a), np.abs(dk)) + np.abs(img["mw"][i])) @ np.abs(A))
        out[5].append(2.0 * np.einsum("tm,mtq->mq", np.abs(beta), np.abs(dk)) @ np.abs(A))
    return [np.array(o) for o in out]


def np_phi_grad(mean, var, dmean, dvar, U, y, mode, Gamma, prior_mean, prior_cov):
    """phi (M,) and grad phi (M, p) at the states U (p, M) in likelihood mode 'gamma' | 'var' | 'gamma_var'."""
    d = mean - y[:, None]
    if mode == "gamma":
        a = np.linalg.solve(Gamma, d)
        s = (d * a).sum(0)
        grad = np.einsum("im,imq->mq", a, dmean)
    else:
        v = var + (np.diag(Gamma)[:, None] if mode == "gamma_var" else 0.0)
        s = (d * d / v + np.log(v)).sum(0)
        grad = np.einsum("im,imq->mq", d / v, dmean) + np.einsum("im,imq->mq", 0.5 * (1 / v - d * d / (v * v)), dvar)
    e = U - prior_mean[:, None]
    w = np.linalg.solve(prior_cov, e)
    return 0.5 * (s + (e * w).sum(0)), grad + w.T


def np_chains_langevin(enka, gps, y, prior, scales, U0, steps, mode, Gamma, nugget, seed, correction=True, beta_via="Li",
                       round32=False, trace=False):
    """Vectorised numpy restatement of gp_mh(chains=M, update='langevin') over the columns (the draws of noise='numpy').
    correction=False drops the Langevin correction from the test (a wrong sampler: the power check of the stationarity test);
    round32 rounds the state to fp32 after every step, as an fp32 engine stores it."""
    rng_state = np.random.get_state()
    np.random.seed(seed)

    def score(U):
        m, v, dm, dv, _, _ = np_predict_grad(enka, gps, U.T, nugget, beta_via)
        ph, grad = np_phi_grad(m, v, dm, dv, U, y, mode, Gamma, np.asarray(prior.mean), np.asarray(prior.cov))
        return ph, scales.T @ grad.T                                             # g = S^T grad phi, (p, M)

    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if round32 else (lambda a: a)
    U = rnd(U0.copy())
    ph, g = score(U)
    acc = np.zeros(U.shape[1])
    kept = []
    for _ in range(steps):
        xi = np.random.normal(0, 1, U.shape)
        lu = np.log(np.random.uniform(size=U.shape[1]))
        P = rnd(U + scales @ (xi - 0.5 * g))
        pp, gp = score(P)
        back = xi - 0.5 * (g + gp)
        corr = 0.5 * (xi * xi).sum(0) - 0.5 * (back * back).sum(0) if correction else 0.0
        with np.errstate(invalid="ignore"):
            t = lu < ph - pp + corr
        U[:, t], ph[t], g[:, t] = P[:, t], pp[t], gp[:, t]
        acc += t
        if trace:
            kept.append(U.copy())
    np.random.set_state(rng_state)
    if trace:
        return U, acc / steps, np.array(kept)
    return U, acc / steps


def linear_emulator(A, b_noise, p, n):
    """_linear_emulator of test_gpu_gp.py: GPs whose Linear mean is the map and whose kernel variance is negligible, so that
    the emulated posterior in mode gamma is an exact Gaussian."""
    from ces_amd import emulate as em
    rng = np.random.default_rng(0)
    U = rng.standard_normal((p, 20))
    G = A @ U
    enka = Enka(p, n, U, G)
    gps = []
    for i in range(n):
        m = em.GPR(U.T, G[i][:, None], em.RBF(input_dim=p, variance=1e-14), mean_function=em.Linear(A[i][:, None], [0.0]))
        m.likelihood.variance = b_noise[i]
        gps.append(m)
    enka.gpmodels = gps
    return enka


def gaussian_problem(M, seed=42):
    """The linear-Gaussian problem of test_gpu_gp.py's stationarity test in mode gamma: (enka with Ustar = M exact posterior
    draws, prior, y, Gamma, posterior mean, posterior covariance)."""
    from scipy import stats
    p, n = 2, 6
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, p))
    sn2 = 0.05 + 0.05 * rng.random(n)
    gam = 0.04 + 0.04 * rng.random(n)
    enka = linear_emulator(A, sn2, p, n)
    mu, C = np.array([0.3, -0.2]), np.array([[1.0, 0.2], [0.2, 0.7]])
    prior = stats.multivariate_normal(mean=mu, cov=C)
    y = A @ np.array([0.5, 0.1]) + 0.1 * rng.standard_normal(n)
    Cp = np.linalg.inv(A.T @ np.diag(1 / gam) @ A + np.linalg.inv(C))
    mp = Cp @ (A.T @ (y / gam) + np.linalg.solve(C, mu))
    enka.Ustar = mp[:, None] + np.linalg.cholesky(Cp) @ rng.standard_normal((p, M))
    return enka, prior, y, np.diag(gam), mp, Cp


def gaussian_bounds_ok(Uf, mp, Cp):
    """Pooled mean within 5 sqrt(C_ii / M) and covariance entries within 5 sqrt((C_ii C_jj + C_ij^2) / M) of the exact ones:
    (ok, worst mean z, worst covariance z)."""
    M = Uf.shape[1]
    zm = np.abs(Uf.mean(axis=1) - mp) / np.sqrt(np.diag(Cp) / M)
    zc = np.abs(np.cov(Uf) - Cp) / np.sqrt((np.outer(np.diag(Cp), np.diag(Cp)) + Cp ** 2) / M)
    return bool(np.all(zm < 5) and np.all(zc < 5)), float(zm.max()), float(zc.max())
