"""Shared cases of model_mh(update='langevin') (tests/test_map_langevin_host.py, tests/test_gpu_map_langevin.py), built on
tests/map_cases.py: the random walk's problems (``problem(kind, None)``: a dense prior covariance, elliptic with its diagonal
Gamma, banana with its dense one), the Langevin steps, the vectorised fp64 numpy chains from the host classes alone, the
Jacobians' sum|terms| and the grid quadrature of the banana posterior."""
import numpy as np

import map_cases as mc_

# the Langevin steps: accept rates 0.77 (elliptic) and 0.66 (banana) over 20 steps of 1 024 chains in fp64 numpy
DELTA = {"elliptic": 1.4, "banana": 0.5}
ENTRY_POINTS = ("cesx_map_jac", "cesx_mh_langevin_start", "cesx_mh_langevin_propose", "cesx_mh_langevin_accept",
                "cesx_mh_langevin_run_map")


def scales(kind):
    """S = delta chol(cov(the 130-particle start ensemble)): what model_mh forms from enka.Ustar."""
    return DELTA[kind] * np.linalg.cholesky(np.cov(mc_.start_ensemble(kind, 130, np.random.default_rng(4))))


def np_map(model, U):
    """The noise-free map of a (2, J) block in fp64 numpy (the host banana class takes one particle per call and draws)."""
    u1, u2 = U
    if model.model_name == "elliptic":
        return np.stack([u2 * x + np.exp(-u1) * (-x ** 2 + x) * 0.5 for x in (model.x1, model.x2)])
    return np.stack([u1 * model.a, u2 / model.a - model.b * (u1 ** 2 + model.a ** 2)])


def jac_abs_terms(model, U):
    """Per entry of DG the sum of the absolute values of the products that form it: (2, 2, J)."""
    u1, u2 = U
    one = np.ones_like(u1)
    if model.model_name == "elliptic":
        e = np.exp(-u1)
        return np.array([[np.abs(e * (-x ** 2 + x) * 0.5), np.abs(x) * one] for x in (model.x1, model.x2)])
    return np.array([[np.abs(model.a) * one, 0.0 * one], [np.abs(2.0 * model.b * u1), np.abs(1.0 / model.a) * one]])


def np_phi_g(prob, S, U):
    """(phi, g = S^T grad phi) of the columns of U: phi with the prior term, grad phi = DG^T Gamma^{-1} (G - y) +
    cov^{-1} (u - mean)."""
    model, y, Gamma, mean, cov, _ = prob
    d = np_map(model, U) - y[:, None]
    a = np.linalg.solve(Gamma, d)
    w = np.linalg.solve(cov, U - mean[:, None])
    phi = 0.5 * (d * a).sum(axis=0) + 0.5 * ((U - mean[:, None]) * w).sum(axis=0)
    grad = np.einsum("iqj,ij->qj", model.jacobian(U), a) + w
    return phi, S.T @ grad


def np_chains_mala(kind, S, U0, steps, seed, correction=True):
    """``steps`` Langevin steps of the M = U0.shape[1] chains in vectorised fp64 numpy: per step
    ``np.random.normal(0, 1, [p, M])``, then ``np.log(np.random.uniform(size=M))`` (the order of ``noise='numpy'``).
    ``seed`` None: the global RNG as it stands.  ``correction=False``: the Langevin proposal under the random walk's test (the
    failing control of the invariance test).  Returns (U, accepted per chain)."""
    prob = mc_.problem(kind, None)
    if seed is not None:
        np.random.seed(seed)
    U = np.array(U0, dtype=np.float64)
    p, M = U.shape
    phi, g = np_phi_g(prob, S, U)
    acc = np.zeros(M, dtype=np.int64)
    for _ in range(steps):
        xi = np.random.normal(0, 1, [p, M])
        logu = np.log(np.random.uniform(size=M))
        P = U + S @ (xi - 0.5 * g)
        php, gp = np_phi_g(prob, S, P)
        back = xi - 0.5 * (g + gp)
        corr = 0.5 * (xi * xi).sum(axis=0) - 0.5 * (back * back).sum(axis=0) if correction else 0.0
        with np.errstate(invalid="ignore"):
            ok = logu < phi - php + corr
        U[:, ok], phi[ok], g[:, ok] = P[:, ok], php[ok], gp[:, ok]
        acc += ok
    return U, acc


def banana_quadrature(n=2001, box=((-4.0, 4.5), (-9.0, 5.0))):
    """Mean (2,) and variances (2,) of exp(-phi) of the banana problem by the trapezoidal rule on an n x n grid."""
    prob = mc_.problem("banana", None)
    x, yv = np.linspace(*box[0], n), np.linspace(*box[1], n)
    X, Y = np.meshgrid(x, yv, indexing="ij")
    model, y, Gamma, mean, cov, _ = prob
    U = np.stack([X.ravel(), Y.ravel()])
    d, c = np_map(model, U) - y[:, None], U - mean[:, None]
    phi = 0.5 * (d * np.linalg.solve(Gamma, d)).sum(axis=0) + 0.5 * (c * np.linalg.solve(cov, c)).sum(axis=0)
    w = np.exp(-(phi - phi.min())).reshape(n, n)
    w[0, :] *= 0.5; w[-1, :] *= 0.5; w[:, 0] *= 0.5; w[:, -1] *= 0.5      # noqa: E702
    w /= w.sum()
    mean = np.array([(w * X).sum(), (w * Y).sum()])
    var = np.array([(w * (X - mean[0]) ** 2).sum(), (w * (Y - mean[1]) ** 2).sum()])
    return mean, var


def moment_z(U, mean, var):
    """z scores of the sample mean and of the second central moments (about the quadrature's mean) of the states U (2, M)
    against the quadrature's, each with the standard error estimated from the sample: (z of the means, z of the variances)."""
    M = U.shape[1]
    d = U - mean[:, None]
    zm = np.abs(d.mean(axis=1)) / (U.std(axis=1, ddof=1) / np.sqrt(M))
    sq = d * d
    zv = np.abs(sq.mean(axis=1) - var) / (sq.std(axis=1, ddof=1) / np.sqrt(M))
    return zm, zv
