"""Shared cases of the closed-form maps' tests (tests/test_maps_host.py, tests/test_gpu_maps.py): the problems, the fp64 numpy
references and the bounds, all computed on the host from the host classes of ces_amd.utils alone."""
import numpy as np

EPS = {"float64": 2.0 ** -52, "float32": 2.0 ** -23}

# elliptic.ipynb: the data, Gamma = 0.1^2 I, the prior N(0, 100 I)
ELLIPTIC_Y = np.array([27.45194112300398, 79.70194112300398])
ELLIPTIC_GAMMA = 0.1 ** 2 * np.identity(2)
BANANA_Y = np.array([0.3, -0.4])
# pCN steps sqrt(beta) chol(prior cov) xi after the shrink sqrt(1 - beta^2) u: elliptic's posterior is ~0.1 wide around u2 = 104.5
# under a prior 5 wide, so a step that is ever accepted needs a small beta
BETA = {"elliptic": 1e-4, "banana": 0.1}


def as_engine(U, dtype):
    """U as the engine holds it (rounded to the engine dtype), in fp64."""
    return np.asarray(U, dtype=np.float64).astype(dtype).astype(np.float64)


def draw_U(kind, J, rng):
    """Columns around the notebooks' ranges: elliptic u1 ~ N(0, 1.5), u2 ~ U(90, 110); banana within a few units."""
    if kind == "elliptic":
        return np.vstack([rng.normal(0.0, 1.5, J), rng.uniform(90.0, 110.0, J)])
    return np.vstack([rng.uniform(-2.5, 2.5, J), rng.uniform(-4.0, 4.0, J)])


def host_columns(model, U):
    """The host class, one column per call (banana takes no blocks), fp64: (n_obs, J)."""
    return np.stack([np.asarray(model(U[:, j]), dtype=np.float64) for j in range(U.shape[1])], axis=1)


def abs_terms(model, U):
    """Per entry of G the sum of the absolute values of the products that form it: (2, J)."""
    u1, u2 = U
    if model.model_name == "elliptic":
        e = np.exp(-u1)
        return np.stack([np.abs(u2 * x) + np.abs(e * (-x ** 2 + x) * 0.5) for x in (model.x1, model.x2)])
    a, b = model.a, model.b
    return np.stack([np.abs(u1 * a), np.abs(u2 / a) + np.abs(b * u1 ** 2) + np.abs(b * a ** 2) + 0.0 * u1])


def problem(kind, update):
    """(model, y, Gamma, prior mean, prior cov, update): elliptic with its diagonal Gamma, banana with its dense one; the
    random walk with a dense prior covariance, pCN with the notebook's diagonal one."""
    from ces_amd import utils
    if kind == "elliptic":
        model, y, Gamma = utils.elliptic(), ELLIPTIC_Y, ELLIPTIC_GAMMA
        mean = np.array([0.0, 100.0])
        cov = np.array([[4.0, 1.5], [1.5, 30.0]]) if update is None else np.diag([4.0, 30.0])
    else:
        model, y = utils.banana(), BANANA_Y
        Gamma = model.Gamma
        mean = np.array([0.2, -0.1])
        cov = np.array([[2.0, 0.6], [0.6, 3.0]]) if update is None else np.diag([2.0, 3.0])
    return model, y, Gamma, mean, cov, update


def start_ensemble(kind, J, rng):
    """An ensemble near the posterior's bulk (phi of order one: proposals are accepted and rejected alike)."""
    if kind == "elliptic":
        # G(u) = y at u = (-2.65.., 104.5..): a cloud around it
        return np.vstack([-2.65 + 0.05 * rng.standard_normal(J), 104.5 + 0.05 * rng.standard_normal(J)])
    return np.vstack([0.3 + 0.4 * rng.standard_normal(J), 0.2 + 0.6 * rng.standard_normal(J)])


def phi_numpy(prob, U):
    """(phi, sum|terms|) of the columns of U in fp64 numpy: phi = 1/2 |L_Gamma^{-1}(g - y)|^2 [+ 1/2 |L_Sigma^{-1}(u - mu)|^2
    for the random walk].  sum|terms|: phi expanded into monomials of the map's own products, y, u and mu, every monomial
    taken by its absolute value -- what a rounding of any intermediate can be amplified by."""
    model, y, Gamma, mean, cov, update = prob
    G = host_columns(model, U)
    Li = np.linalg.inv(np.linalg.cholesky(Gamma))
    d = Li @ (G - y[:, None])
    phi = 0.5 * (d * d).sum(axis=0)
    mag = 0.5 * ((np.abs(Li) @ (abs_terms(model, U) + np.abs(y)[:, None])) ** 2).sum(axis=0)
    if update is None:
        Ls = np.linalg.inv(np.linalg.cholesky(cov))
        w = Ls @ (U - mean[:, None])
        phi = phi + 0.5 * (w * w).sum(axis=0)
        mag = mag + 0.5 * ((np.abs(Ls) @ (np.abs(U) + np.abs(mean)[:, None])) ** 2).sum(axis=0)
    return phi, mag
