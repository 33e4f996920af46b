"""The Emulate stage on the device: cesx_gp_predict against the fp64 numpy restatement, MCMC.gp_mh(chains=) against the
real reference's chains (tests/golden/gp_mcmc.npz) and a vectorised numpy restatement, its stationarity at 65 536
chains, bit-identical device-noise runs and exact resumes."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import Enka, build_gps, gold_call, gold_prior, gold_problem, load_gold  # noqa: E402
from gp_cases import random_gps  # noqa: E402,F401  (test_gpu_emulate_edges.py takes it from here)

pytestmark = pytest.mark.gpu
FAMILIES = ["RBF", "Matern12", "Matern32", "Matern52"]


def np_predict(enka, gps, X, nugget=True):
    """fp64 numpy restatement with its bars: (mean, var, sum |alpha_j k_j| per point, sigma^2 per GP)."""
    from ces_amd import emulate as em
    img = em.device_image(enka, gps)
    means, vars_, scale = [], [], []
    for i, m in enumerate(gps):
        Z = (img["A"][i] @ (X.T - img["c"][:, None])).T
        kern = m.kern
        d = Z[:, None, :] - img["Z"][i][None, :, :]
        Ks = kern.variance * kern.f(np.sqrt((d * d).sum(-1)))                   # (M, Jt)
        a = img["alpha"][i]
        means.append(Ks @ a + Z @ img["mw"][i] + img["par"][i, 2])
        W = img["Li"][i] @ Ks.T
        vars_.append(kern.variance - (W * W).sum(0) + (m.likelihood.variance if nugget else 0.0))
        scale.append(np.abs(Ks * a).sum(1) + np.abs(Z @ img["mw"][i]) + abs(img["par"][i, 2]))
    return np.array(means), np.array(vars_), np.array(scale), img["par"][:, 0]


def device_predict(enka, X, nugget=True, var=True, dtype="float64"):
    from ces_amd import emulate as em
    from ces_amd import engine
    img = em.device_image(enka, enka.gpmodels)
    eng = engine.Engine(X.shape[1], img["n"], X.shape[0], dtype=dtype)
    eng.gp_set(img)
    Xd = eng.to_device(np.ascontiguousarray(X.T), X.shape[1], "gp_X")
    m, v = eng.gp_predict(Xd, nugget=nugget, var=var)
    Xh = eng.to_host(Xd).T.astype(np.float64)
    return m.cpu().numpy(), (None if v is None else v.cpu().numpy()), Xh


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("scaled", [False, True])
def test_predict_against_numpy(family, scaled):
    rng = np.random.default_rng(hash((family, scaled)) % 2**32)
    p, n, Jt, M = 3, 5, 77, 203                         # ragged J_t and M
    enka = random_gps(rng, p, n, Jt, family, scaled)
    X = np.vstack([enka.Ustar.T, rng.standard_normal((M - Jt, p))])     # the first Jt queries on the training inputs
    for nugget in (True, False):
        m, v, Xh = device_predict(enka, X, nugget)
        mr, vr, sc, s2 = np_predict(enka, enka.gpmodels, Xh, nugget)
        assert np.all(np.abs(m - mr) <= 1e-9 * (sc + 1e-300)), np.max(np.abs(m - mr) / sc)
        assert np.all(np.abs(v - vr) <= 1e-9 * s2[:, None]), np.max(np.abs(v - vr) / s2[:, None])
    mo, vo, _ = device_predict(enka, X, True, var=False)
    assert vo is None and np.array_equal(mo, m)


def test_predict_fitted_emulator_host_and_device_agree():
    from ces_amd import emulate as em
    rng = np.random.default_rng(8)
    U = rng.standard_normal((2, 60))
    enka = Enka(2, 3, U, np.vstack([U[0] + 0.2 * U[1] ** 2, np.sin(U[1]), U.sum(0)]))
    em.train_gps(enka, kernel="Matern32", mean_function="Linear", maxiter=300)
    X = np.vstack([U.T[:10], rng.standard_normal((90, 2))])
    for nugget in (True, False):
        hm, hv = em.predict_gps(enka, X, nugget=nugget)
        dm, dv = em.predict_gps(enka, X, nugget=nugget, device=True)
        mr, vr, sc, s2 = np_predict(enka, enka.gpmodels, X, nugget)
        assert np.all(np.abs(dm - hm) <= 1e-9 * sc)
        assert np.all(np.abs(dv - hv) <= 1e-9 * s2[:, None] + 1e-9 * np.abs(hv))


@pytest.mark.parametrize("Jt,p,M", [(1, 1, 5), (16, 1, 33), (700, 2, 70), (2048, 4, 64)])
def test_predict_shapes(Jt, p, M):
    rng = np.random.default_rng(Jt)
    enka = random_gps(rng, p, 2, Jt, "Matern52", mean="Constant")
    X = np.vstack([enka.Ustar.T[:min(Jt, M)], rng.standard_normal((max(0, M - Jt), p))])[:M]
    m, v, Xh = device_predict(enka, X, True, dtype="float32")
    mr, vr, sc, s2 = np_predict(enka, enka.gpmodels, Xh, True)
    assert np.all(np.abs(m - mr) <= 1e-9 * sc)
    assert np.all(np.abs(v - vr) <= 1e-9 * s2[:, None])


def _gold_device(c, a, man, dtype="float64"):
    from ces_amd import sample
    enka = gold_problem(a, c["scaled"])
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    mc.engine_dtype = dtype
    np.random.seed(c["seed"])
    call = gold_call(a, c["kwargs"])
    if c["resume"]:
        mc.gp_mh(enka, c["resume"], gold_prior(a), chains=1, **call)
        mc.gp_mh(enka, man["STEPS"] - c["resume"], gold_prior(a), chains=1, **call)
    else:
        mc.gp_mh(enka, man["STEPS"], gold_prior(a), chains=1, **call)
    return mc


DEVICE_CASES = [c["name"] for c in load_gold()[0]["cases"] if c["name"] not in ("pca", "compounded_dense")]


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_chains1_reproduces_reference(case):
    man, a = load_gold()
    c = [c for c in man["cases"] if c["name"] == case][0]
    mc = _gold_device(c, a, man)
    np.testing.assert_allclose(mc.samples, a["mh_%s_samples" % case], rtol=1e-10, atol=1e-10)
    assert abs(mc.accept - float(a["mh_%s_accept" % case])) < 1e-12


def np_chains(enka, gps, y, prior, scales, U0, steps, mode, Gamma, nugget, seed, update=None, beta=0.5):
    """Vectorised numpy restatement of gp_mh over the columns (the draws of noise='numpy')."""
    rng_state = np.random.get_state()
    np.random.seed(seed)
    Si = np.linalg.inv(prior.cov)

    def phi(U):
        m, v, _, _ = np_predict(enka, gps, U.T, nugget)
        d = m - y[:, None]
        if mode == "gamma":
            s = (d * np.linalg.solve(Gamma, d)).sum(0)
        else:
            S = v + (np.diag(Gamma)[:, None] if mode == "gamma_var" else 0.0)
            s = (d * d / S + np.log(S)).sum(0)
        e = U - prior.mean[:, None]
        return 0.5 * (s + (e * (Si @ e)).sum(0))

    U = U0.copy()
    ph = phi(U)
    acc = np.zeros(U.shape[1])
    a_, b_ = (np.sqrt(1 - beta ** 2), np.sqrt(beta)) if update == "pCN" else (1.0, 1.0)
    for _ in range(steps):
        xi = np.random.normal(0, 1, U.shape)
        lu = np.log(np.random.uniform(size=U.shape[1]))
        P = a_ * U + b_ * scales @ xi
        pp = phi(P)
        t = lu < ph - pp
        U[:, t], ph[t] = P[:, t], pp[t]
        acc += t
    np.random.set_state(rng_state)
    return U, acc / steps


@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_1024_chains_against_numpy(mode, dtype):
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    prior = gold_prior(a)
    Gamma = a["prob_Gamma_diag"] if mode != "var" else None
    kw = dict(Gamma=Gamma) if Gamma is not None else {}
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    M, steps = 1024, 20
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    mc.engine_dtype = dtype
    mc.trace_stride = steps
    np.random.seed(5)
    mc.gp_mh(enka, steps, prior, chains=M, start="ensemble" if M <= 30 else "mean", **kw)
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    scales = np.linalg.cholesky(np.cov(enka.Ustar))
    Ur, rate = np_chains(enka, enka.gpmodels, a["prob_y"], prior, scales, U0, steps, mode,
                         Gamma if Gamma is not None else np.eye(4), True, 5)
    Ud = mc.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    assert agree.mean() > (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(mc.accept - rate.mean()) < (1e-12 if dtype == "float64" else 0.01)


def test_start_on_training_points():
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    mc.noise = "device"
    mc.gp_mh(enka, 5, gold_prior(a), chains=30, start="ensemble")
    assert mc.samples.shape == (2, 6, 30) and np.array_equal(mc.samples[:, 0, :], enka.Ustar)
    assert np.all(np.isfinite(mc.samples))


def _linear_emulator(A, b_noise, p, n):
    """GPs whose Linear mean is the map (alpha = 0: the outputs equal the mean at every training point) and whose kernel
    variance is negligible; with the nugget the variance is the likelihood variance."""
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


@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var"])
def test_stationarity_at_65536_chains(mode):
    from ces_amd import sample
    p, n, M = 2, 6, 65536
    rng = np.random.default_rng(42)
    A = rng.standard_normal((n, p))
    sn2 = 0.05 + 0.05 * rng.random(n)
    gam = 0.04 + 0.04 * rng.random(n)
    enka = _linear_emulator(A, sn2, p, n)
    mu, C = np.array([0.3, -0.2]), np.array([[1.0, 0.2], [0.2, 0.7]])
    prior = stats.multivariate_normal(mean=mu, cov=C)
    y = A @ np.array([0.5, 0.1]) + 0.1 * rng.standard_normal(n)
    noise = dict(gamma=gam, var=sn2, gamma_var=gam + sn2)[mode]
    kw = {} if mode == "var" else dict(Gamma=np.diag(gam))
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    # the analytic posterior (the log det terms are constant in u here)
    Pi = A.T @ np.diag(1 / noise) @ A + np.linalg.inv(C)
    Cp = np.linalg.inv(Pi)
    mp = Cp @ (A.T @ (y / noise) + np.linalg.solve(C, mu))
    # chains start from the posterior itself: stationarity means they stay there
    L = np.linalg.cholesky(Cp)
    U0 = mp[:, None] + L @ rng.standard_normal((p, M))
    enka.Ustar = U0                                        # start='ensemble' reads Ustar; the scales chol(cov(Ustar))
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = y
    mc.noise = "device"
    mc.trace_stride = 50
    mc.gp_mh(enka, 50, prior, chains=M, start="ensemble", **kw)
    Uf = mc.samples[:, -1, :]
    z = (Uf.mean(axis=1) - mp) / np.sqrt(np.diag(Cp) / M)
    assert np.all(np.abs(z) < 5), z
    ratio = Uf.var(axis=1) / np.diag(Cp)
    assert np.all(np.abs(ratio - 1) < 0.05), ratio
    assert 0.2 < mc.accept < 0.95


def test_device_noise_bit_identical_and_exact_resume():
    from ces_amd import sample
    man, a = load_gold()

    def run(splits):
        enka = gold_problem(a)
        mc = sample.MCMC()
        mc.mute_bar = True
        mc.y_obs = a["prob_y"]
        mc.noise = "device"
        mc.seed = 99
        for s in splits:
            mc.gp_mh(enka, s, gold_prior(a), chains=257)
        return mc.samples
    one = run([40])
    assert np.array_equal(one, run([40]))
    two = run([25, 15])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
