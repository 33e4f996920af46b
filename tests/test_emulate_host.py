"""The Emulate stage on the host (ces_amd/emulate.py) and the host GP sampler (MCMC.gp_mh): the GPR against a literal
dense-inverse restatement, its gradient and fit, and chains / predictions of the real reference's ces/emulate.py and
ces/sample.py (tests/golden/gp_mcmc.npz, written by tools/make_golden_gp.py)."""
import json
import os
import sys

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GP_ENTRY_POINTS = ("cesx_gp_set", "cesx_gp_predict", "cesx_gp_start", "cesx_gp_accept")
FAMILIES = ["RBF", "Matern12", "Matern32", "Matern52"]


def load_gold():
    with open(os.path.join(GOLD, "gp_mcmc_manifest.json")) as fh:
        man = json.load(fh)
    return man, dict(np.load(os.path.join(GOLD, "gp_mcmc.npz")))


class Enka(object):
    """The attributes of an enka that the Emulate and Sample stages read."""

    def __init__(self, p, n_obs, Ustar, Gstar):
        self.p, self.n_obs, self.Ustar, self.Gstar = p, n_obs, Ustar, Gstar


def build_gps(X, Gstar, hyp, family="Matern32", mean="Linear"):
    from ces_amd import emulate as em
    Kern = getattr(em, family)
    gps = []
    for i in range(Gstar.shape[0]):
        k = Kern(input_dim=X.shape[1], ARD=True, lengthscales=hyp["ls"][i], variance=hyp["var"][i])
        if mean == "Linear":
            mf = em.Linear(hyp["mA"][i].reshape(-1, 1), [hyp["mb"][i]])
        elif mean == "Constant":
            mf = em.Constant([hyp["mb"][i]])
        else:
            mf = None
        m = em.GPR(X, Gstar[i][:, None], k, mean_function=mf)
        m.likelihood.variance = hyp["lik"][i]
        gps.append(m)
    return gps


def gold_problem(a, scaled=False, family="Matern32", mean="Linear"):
    Ustar, Gstar = a["prob_Ustar"], a["prob_Gstar"]
    hyp = {k[len("prob_hyp_"):]: v for k, v in a.items() if k.startswith("prob_hyp_")}
    enka = Enka(Ustar.shape[0], Gstar.shape[0], Ustar, Gstar)
    X = Ustar.T
    if scaled:
        enka.scale = {"mean": Ustar.mean(axis=1)[:, None], "cov": 2.0 * np.linalg.cholesky(np.cov(Ustar))}
        enka.scaled = True
        X = np.linalg.solve(enka.scale["cov"], Ustar - enka.scale["mean"]).T
    enka.gpmodels = build_gps(X, Gstar, hyp, family, mean)
    return enka


def gold_call(a, kw):
    call = {k: v for k, v in kw.items() if k not in ("Gamma", "pca")}
    if "Gamma" in kw:
        call["Gamma"] = a["prob_Gamma_" + kw["Gamma"]]
    if kw.get("pca"):
        call["pca_tools"] = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    return call


def gold_prior(a):
    return stats.multivariate_normal(mean=a["prob_mu"], cov=a["prob_Sigma"])


def dense_predict(X, Y, kfun, mfun, sn2, Xq):
    """The predictive equations with a literal dense inverse."""
    K = kfun(X, X) + sn2 * np.eye(len(X))
    Ki = np.linalg.inv(K)
    Ks = kfun(X, Xq)
    mean = Ks.T @ Ki @ (Y - mfun(X)) + mfun(Xq)
    var = np.diag(kfun(Xq, Xq)) - np.einsum("ij,ik,kj->j", Ks, Ki, Ks)
    return mean, var[:, None]


def literal_kernel(family, var, ls):
    def k(A, B):
        r = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2 / ls ** 2).sum(-1))
        if family == "RBF":
            return var * np.exp(-0.5 * r ** 2)
        if family == "Matern12":
            return var * np.exp(-r)
        if family == "Matern32":
            return var * (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)
        return var * (1 + np.sqrt(5) * r + 5 * r ** 2 / 3) * np.exp(-np.sqrt(5) * r)
    return k


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mean", ["Zero", "Constant", "Linear"])
def test_gpr_against_dense_inverse(family, mean):
    from ces_amd import emulate as em
    rng = np.random.default_rng(3)
    X = rng.standard_normal((25, 3))
    Y = np.sin(X).sum(axis=1, keepdims=True)
    Xq = np.vstack([X[:4], rng.standard_normal((6, 3))])
    ls, var, sn2 = np.array([0.7, 1.2, 0.9]), 0.8, 1e-3
    if mean == "Zero":
        mf, mfun = None, lambda Z: np.zeros((len(Z), 1))
    elif mean == "Constant":
        mf, mfun = em.Constant([0.3]), lambda Z: np.full((len(Z), 1), 0.3)
    else:
        Am, bm = np.array([[0.5], [-0.2], [0.1]]), 0.2
        mf, mfun = em.Linear(Am, [bm]), lambda Z: Z @ Am + bm
    m = em.GPR(X, Y, getattr(em, family)(input_dim=3, ARD=True, lengthscales=ls, variance=var), mean_function=mf)
    m.likelihood.variance = sn2
    mu, v = m.predict_f(Xq)
    mu_r, v_r = dense_predict(X, Y, literal_kernel(family, var, ls), mfun, sn2, Xq)
    assert mu.shape == (10, 1) and v.shape == (10, 1)
    np.testing.assert_allclose(mu, mu_r, rtol=0, atol=1e-10 * max(1.0, np.abs(mu_r).max()))
    np.testing.assert_allclose(v, v_r, rtol=0, atol=1e-10 * var)
    my, vy = m.predict_y(Xq)
    np.testing.assert_array_equal(my, mu)
    np.testing.assert_allclose(vy, v + sn2, rtol=0, atol=1e-15)


def test_kernel_defaults_and_shapes():
    from ces_amd import emulate as em
    k = em.Matern32(input_dim=2)
    assert k.variance == 1.0 and k.lengthscales == 1.0 and not k.ARD
    k = em.RBF(input_dim=3, ARD=True)
    assert np.array_equal(k.lengthscales, np.ones(3))
    m = em.GPR(np.zeros((3, 2)) + np.arange(3)[:, None], np.arange(3.0)[:, None], em.Matern52(input_dim=2))
    assert m.likelihood.variance == 1.0
    # r is exactly 0 on a training point: k(x, x) = variance
    assert m.kern.K(m.X)[1, 1] == m.kern.variance


@pytest.mark.parametrize("family", FAMILIES)
def test_lml_gradient_central_differences(family):
    from ces_amd import emulate as em
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2))
    Y = np.cos(X[:, :1]) + 0.1 * X[:, 1:]
    m = em.GPR(X, Y, getattr(em, family)(input_dim=2, ARD=True, lengthscales=[0.8, 1.4], variance=0.7),
               mean_function=em.Linear(np.array([[0.2], [0.1]]), [0.05]))
    m.likelihood.variance = 0.05
    lml, g = m.log_marginal_likelihood_and_grad()
    assert abs(lml - m.log_marginal_likelihood()) < 1e-10
    pos, free = m._get()
    x0 = np.concatenate([pos, free])
    num = np.zeros_like(x0)
    for i in range(len(x0)):
        h = 1e-6 * max(1.0, abs(x0[i]))
        for sgn in (1, -1):
            x = x0.copy()
            x[i] += sgn * h
            m._set(x[:len(pos)], x[len(pos):])
            num[i] += sgn * m.log_marginal_likelihood() / (2 * h)
    m._set(pos, free)
    np.testing.assert_allclose(g, num, rtol=1e-5, atol=1e-6)


def test_fit_raises_lml_and_recovers_lengthscales():
    from ces_amd import emulate as em
    rng = np.random.default_rng(11)
    X = rng.uniform(-3, 3, size=(200, 2))
    true_ls = np.array([0.8, 3.0])
    k_true = em.RBF(input_dim=2, ARD=True, lengthscales=true_ls, variance=1.0)
    K = k_true.K(X) + 1e-4 * np.eye(200)
    Y = np.linalg.cholesky(K) @ rng.standard_normal((200, 1))
    m = em.GPR(X, Y, em.RBF(input_dim=2, ARD=True))
    before = m.log_marginal_likelihood()
    em.ScipyOptimizer().minimize(m, maxiter=500)
    assert m.log_marginal_likelihood() > before + 10
    np.testing.assert_allclose(m.kern.lengthscales, true_ls, rtol=0.35)
    assert m.likelihood.variance >= em.FLOOR


def test_train_gps_is_the_notebook_emulate():
    from ces_amd import emulate as em
    rng = np.random.default_rng(2)
    U = rng.standard_normal((2, 40))
    G = np.vstack([U[0] + 0.3 * np.sin(U[1]), U[1] ** 2])
    enka = Enka(2, 2, U, G)
    gps = em.train_gps(enka, kernel="Matern32", maxiter=200)
    assert gps is enka.gpmodels and len(gps) == 2
    assert all(isinstance(m.kern, em.Matern32) and m.kern.ARD for m in gps)
    mean, var = em.predict_gps(enka, U.T[:5])
    assert np.abs(mean - G[:, :5]).max() < 0.1 and np.all(var > 0)


def test_predict_gps_fixtures():
    from ces_amd import emulate as em
    man, a = load_gold()
    Xq = a["pred_X"]
    for c in man["predict"]:
        enka = gold_problem(a, c["scaled"], c["family"], c["mean"])
        m, v = em.predict_gps(enka, Xq, nugget=c["nugget"])
        tag = "pred_%s_%s_%d_%d_" % (c["family"], c["mean"], c["scaled"], c["nugget"])
        np.testing.assert_allclose(m, a[tag + "mean"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(v, a[tag + "var"], rtol=1e-12, atol=1e-12)
    enka = gold_problem(a)
    m, v = em.predict_gps(enka, Xq[:1], pca_tools=dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"]))
    np.testing.assert_allclose(m, a["pred_pca_mean"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(v, a["pred_pca_var"], rtol=1e-12, atol=1e-12)
    assert em.predict_gps(Enka(2, 4, a["prob_Ustar"], a["prob_Gstar"]), Xq) == ''


def test_scale_gppreds_and_scale_ensemble_fixtures():
    from ces_amd import emulate as em
    man, a = load_gold()
    sm, sv = em.scale_gppreds(list(a["sgp_gm"]), list(a["sgp_gv"]), a["sgp_Gm"], a["sgp_Gs"])
    np.testing.assert_allclose(sm, a["sgp_mean"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(sv, a["sgp_var"], rtol=1e-13, atol=0)
    enka = Enka(2, 4, a["prob_Ustar"], a["prob_Gstar"])
    with pytest.raises(AttributeError):
        em.scale_ensemble(enka, factor=1.5)
    assert man["scale_ensemble_error"] == "AttributeError"
    np.testing.assert_allclose(enka.scale["mean"], a["se_mean"], rtol=1e-14)
    np.testing.assert_allclose(enka.scale["cov"], a["se_cov"], rtol=1e-14)


@pytest.mark.parametrize("case", [c["name"] for c in load_gold()[0]["cases"]])
def test_gp_mh_host_reproduces_reference(case):
    from ces_amd import sample
    man, a = load_gold()
    c = [c for c in man["cases"] if c["name"] == case][0]
    enka = gold_problem(a, c["scaled"])
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    np.random.seed(c["seed"])
    call = gold_call(a, c["kwargs"])
    if c["resume"]:
        mc.gp_mh(enka, c["resume"], gold_prior(a), **call)
        mc.gp_mh(enka, man["STEPS"] - c["resume"], gold_prior(a), **call)
    else:
        mc.gp_mh(enka, man["STEPS"], gold_prior(a), **call)
    np.testing.assert_allclose(mc.samples, a["mh_%s_samples" % case], rtol=1e-12, atol=1e-12)
    assert abs(mc.accept - float(a["mh_%s_accept" % case])) < 1e-12


def test_gp_mh_emulator_sources_and_unknown_update():
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    gps = enka.gpmodels
    del enka.gpmodels
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    with pytest.raises(ImportError, match="GPflow"):
        mc.gp_mh(enka, 3, gold_prior(a))
    enka.gpmodels = None                                     # (predict_gps reads the kwarg once enka has the attribute)
    np.random.seed(1)
    mc.gp_mh(enka, 3, gold_prior(a), gpmodels=gps)
    assert mc.samples.shape == (2, 4)
    del mc.samples
    enka.gpmodels = gps
    with pytest.raises(UnboundLocalError):
        mc.gp_mh(enka, 3, gold_prior(a), update="MALA")


@pytest.mark.parametrize("kw,match", [
    (dict(pca="yes"), "pca_tools"),
    (dict(separable=True), "separable"),
    (dict(Gamma="dense", noise_compounded=True), "dense Gamma"),
    (dict(update="MALA"), "unknown update"),
    (dict(chains=0), "chains"),
])
def test_gp_mh_chains_unsupported_options(kw, match):
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    kw = dict(kw)
    if kw.pop("pca", None):
        kw["pca_tools"] = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    if kw.get("Gamma") == "dense":
        kw["Gamma"] = a["prob_Gamma_dense"]
    kw.setdefault("chains", 4)
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    with pytest.raises(ValueError, match=match):
        mc.gp_mh(enka, 2, gold_prior(a), **kw)


def test_gp_mh_chains_rejects_foreign_emulators_and_counts():
    from ces_amd import sample

    class Foreign(object):
        def predict_y(self, X):
            return np.zeros((len(X), 1)), np.ones((len(X), 1))
        predict_f = predict_y

    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    with pytest.raises(ValueError, match="GPR"):
        mc.gp_mh(enka, 2, gold_prior(a), chains=4, gpmodels=[Foreign() for _ in range(4)])
    with pytest.raises(ValueError, match="n_obs"):
        mc.gp_mh(enka, 2, gold_prior(a), chains=4, gpmodels=enka.gpmodels[:3])


def test_gp_abi_declared_exported_no_scratch():
    from ces_amd import engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    for name in GP_ENTRY_POINTS:
        assert name + "(" in hdr and name in engine.EXPORTS
    from ces_amd import build
    assert "kernels_gp.hip" in build.SOURCES
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    t = isa_audit.collect(["kernels_gp.hip"])
    rows = {k: v for k, v in t.items() if "gp_predict_kernel" in k or "gp_score_kernel" in k}
    assert len(rows) == 6                               # predict {float, double} x {LDS, global panel}, score {float, double}
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, name
        assert r["scratch_total"] == 0, name
    assert all(r["mfma_in_loop"] > 0 for k, r in rows.items() if "gp_predict_kernel" in k)
