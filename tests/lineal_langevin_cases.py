"""Shared cases of model_mh(update='langevin') for the linear maps (tests/test_lineal_langevin_host.py,
tests/test_gpu_lineal_langevin.py): seeded problems at the shapes where the update kernels change path, each with a dense and a
diagonal Gamma and Sigma, a 130-particle start ensemble and a step; the fp64 numpy restatement of phi and g = S^T grad phi, the
vectorised numpy chains with the driver's draw order, the elementwise rounding bound of g and the mutants it has to reject."""
import numpy as np

ENTRY_POINTS = ("cesx_mh_langevin_lineal_set", "cesx_mh_langevin_lineal_start", "cesx_mh_langevin_lineal_propose",
                "cesx_mh_langevin_lineal_accept", "cesx_mh_langevin_lineal_g")

# name: (map, p, n, b)   b: 'vector' | 'scalar' | 'zero'
CASES = {
    "lineal-5x3": ("lineal", 5, 3, "vector"),
    "lineal-17x33": ("lineal", 17, 33, "scalar"),        # nothing a multiple of 16
    "lineal-64x64": ("lineal", 64, 64, "vector"),        # whole tiles
    "lineal-65x64": ("lineal", 65, 64, "zero"),          # one row past a tile
    "log-5x3": ("lineal_log", 5, 3, "zero"),
    "log-17x33": ("lineal_log", 17, 33, "zero"),
}
# the Langevin steps: fp64 numpy accept rates over 20 steps of 1 025 chains from the ensemble mean lie in (0.5, 0.95) for every
# form of Gamma and Sigma (printed by test_lineal_langevin_host.py::test_steps_accept_between_half_and_095)
DELTA = {"lineal-5x3": 0.9, "lineal-17x33": 0.8, "lineal-64x64": 0.5, "lineal-65x64": 0.5, "log-5x3": 0.6, "log-17x33": 0.3}
FORMS = [(gd, sd) for gd in (False, True) for sd in (False, True)]      # (dense Gamma, dense Sigma)


def _spd(rng, k, scale):
    M = rng.standard_normal((k, k))
    return scale * (M @ M.T / k + np.eye(k))


def problem(name, gamma_dense, sigma_dense):
    """dict(kind, p, n, A, b, Gamma, Sigma, mu, y, ens (p, 130), delta, m, C): every form of one name shares A, b, mu and the
    draws behind y and the ensemble.  ``m``, ``C``: the exact Gaussian posterior (lineal) or the Laplace approximation at the
    true u (lineal_log), which the ensemble is drawn from."""
    kind, p, n, bk = CASES[name]
    rng = np.random.default_rng(sum(ord(c) for c in name))
    if kind == "lineal":
        A = rng.standard_normal((n, p)) / np.sqrt(p)
    else:
        A = rng.uniform(0.2, 1.0, (n, p)) / p
    b = {"vector": 0.5 * rng.standard_normal(n), "scalar": 0.3, "zero": 0}[bk]
    Gd, Gf = np.diag(rng.uniform(0.05, 0.2, n)), _spd(rng, n, 0.05)
    Sd, Sf = np.diag(rng.uniform(0.5, 2.0, p)), _spd(rng, p, 0.5)
    Gamma, Sigma = (Gf if gamma_dense else Gd), (Sf if sigma_dense else Sd)
    mu = 0.3 * rng.standard_normal(p)
    z_u, z_y, z_e = rng.standard_normal(p), rng.standard_normal(n), rng.standard_normal((p, 130))
    u_true = mu + 0.5 * np.linalg.cholesky(Sigma) @ z_u
    E = np.exp(u_true) if kind == "lineal_log" else u_true
    y = A @ E + b + np.linalg.cholesky(Gamma) @ z_y
    Gi, Si = np.linalg.inv(Gamma), np.linalg.inv(Sigma)
    if kind == "lineal":
        C = np.linalg.inv(A.T @ Gi @ A + Si)
        m = C @ (A.T @ Gi @ (y - b) + Si @ mu)
    else:
        J = A * np.exp(u_true)[None, :]
        C = np.linalg.inv(J.T @ Gi @ J + Si)
        m = u_true
    C = 0.5 * (C + C.T)
    ens = m[:, None] + np.linalg.cholesky(C) @ z_e
    return dict(name=name, kind=kind, p=p, n=n, A=A, b=b, Gamma=Gamma, Sigma=Sigma, mu=mu, y=y, ens=ens, delta=DELTA[name], m=m, C=C)


def scales(prob):
    """S = delta chol(cov(the start ensemble)): what model_mh forms from enka.Ustar."""
    return prob["delta"] * np.linalg.cholesky(np.cov(prob["ens"]).reshape(prob["p"], prob["p"]))


def model_of(prob, gradient=True):
    from ces_amd import utils
    mdl = utils.lineal(prob["A"], prob["b"]) if prob["kind"] == "lineal" else utils.lineal_log(prob["A"])
    return mdl.enable_gradient() if gradient else mdl


def np_map(prob, U):
    E = np.exp(U) if prob["kind"] == "lineal_log" else U
    return prob["A"] @ E + np.reshape(np.broadcast_to(np.asarray(prob["b"], dtype=np.float64), (prob["n"],)), (-1, 1))


def np_phi_g(prob, S, U, G=None, mutant=None):
    """(phi, g = S^T grad phi) of the columns of U in fp64: phi with the prior term, grad phi = DG^T Gamma^{-1} (G - y) +
    Sigma^{-1} (U - mu), DG = A or A diag(exp U).  ``G``: the map's rows where they are not ``np_map(prob, U)`` (an fp32 engine's).
    ``mutant``: one of MUTANTS, a wrong g that the bound of ``g_bound`` has to reject."""
    G = np_map(prob, U) if G is None else G
    d = G - prob["y"][:, None]
    a = np.linalg.solve(prob["Gamma"], d)
    w = np.linalg.solve(prob["Sigma"], U - prob["mu"][:, None])
    phi = 0.5 * (d * a).sum(axis=0) + 0.5 * ((U - prob["mu"][:, None]) * w).sum(axis=0)
    if mutant == "bias_dropped":                           # no -A^T Gamma^{-1} y
        a = np.linalg.solve(prob["Gamma"], G)
    t = prob["A"].T @ a
    if prob["kind"] == "lineal_log" and mutant != "exp_missing":
        t = np.exp(U) * t
    grad = t + (0.0 if mutant == "prior_missing" else w)
    return phi, (S if mutant == "S_not_transposed" else S.T) @ grad


MUTANTS = ("bias_dropped", "prior_missing", "S_not_transposed", "exp_missing")


def g_bound(prob, S, U, dtype):
    """Elementwise c u_T mag for g at the states U:
        mag = |S^T| ( |DG^T| |L_G^{-T}| |L_G^{-1}| (|A| |E| + |b| + |y|) + |L_S^{-T}| |L_S^{-1}| (|U| + |mu|) ),
    E = U or exp(U), DG = A or A diag(exp U); u_T = 2^-24 / 2^-53; c = 2 (n + 2 p) + 16: the chained products have depths p, n, n,
    2 p, p, one rounding per stored operand image and per stored intermediate, and 4 for exp."""
    p, n = prob["p"], prob["n"]
    u = 2.0 ** -24 if str(dtype) in ("float32", "torch.float32") else 2.0 ** -53
    c = 2 * (n + 2 * p) + 16
    LGi = np.abs(np.linalg.inv(np.linalg.cholesky(prob["Gamma"])))
    LSi = np.abs(np.linalg.inv(np.linalg.cholesky(prob["Sigma"])))
    E = np.exp(U) if prob["kind"] == "lineal_log" else np.abs(U)
    bvec = np.abs(np.broadcast_to(np.asarray(prob["b"], dtype=np.float64), (n,)))
    data = LGi.T @ (LGi @ (np.abs(prob["A"]) @ E + (bvec + np.abs(prob["y"]))[:, None]))
    t = np.abs(prob["A"]).T @ data
    if prob["kind"] == "lineal_log":
        t = np.exp(U) * t
    prior = LSi.T @ (LSi @ (np.abs(U) + np.abs(prob["mu"])[:, None]))
    return c * u * (np.abs(S).T @ (t + prior))


def np_chains_mala_lineal(prob, S, U0, steps, seed, correction=True):
    """``steps`` Langevin steps of the M = U0.shape[1] chains in vectorised fp64 numpy: per step
    ``np.random.normal(0, 1, [p, M])``, then ``np.log(np.random.uniform(size=M))`` (the order of ``noise='numpy'``).  ``seed``
    None: the global RNG as it stands.  ``correction=False``: the Langevin proposal under the random walk's test (the failing
    control of the invariance test).  Returns (U, accepted per chain)."""
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


def exact_draws(prob, M, seed):
    """M draws of N(m, C): the exact posterior of a lineal problem."""
    rng = np.random.default_rng(seed)
    return prob["m"][:, None] + np.linalg.cholesky(prob["C"]) @ rng.standard_normal((prob["p"], M))


def moment_z(U, mean, var):
    """z scores of the sample mean and of the second central moments (about ``mean``) of the states U (p, M) against ``mean``
    and ``var``, each with the standard error estimated from the sample: (z of the means, z of the variances)."""
    M = U.shape[1]
    d = U - mean[:, None]
    zm = np.abs(d.mean(axis=1)) / (U.std(axis=1, ddof=1) / np.sqrt(M))
    sq = d * d
    zv = np.abs(sq.mean(axis=1) - var) / (sq.std(axis=1, ddof=1) / np.sqrt(M))
    return zm, zv
