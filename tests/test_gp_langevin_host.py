"""gp_mh(update='langevin') on the host: the closed-form GP gradients and grad phi against central differences, the short
form of the Langevin correction against the two proposal densities written out, the refusals, and the ABI's declarations.

Bars (measured with the formulas right, then a wrong formula shown to miss them by 100 x or more; NOTEBOOK.md):
  grad mean   step 1e-5, |grad - quotient| <= 1e-8 of sum_t |alpha_t| |dk_t| + |w|            (measured 1.2e-10)
  grad var    step 1e-5, |grad - quotient| <= 1e-4 of 2 sum_t |beta_t| |dk_t|                 (measured 1.7e-6: the variance
              bends sharply at a training point, so the quotient's own truncation error sets it; a factor 2 dropped from
              grad var leaves 1.2e-2 or more, A^T omitted 2.0e-2 or more of the mean's bar)
  grad phi    step 1e-5, |grad - quotient| <= 1e-6 of |grad phi|_inf + 1                        (measured 3.1e-8 at most; the prior
              term dropped leaves 6.2e-4 or more, the grad var term dropped 0.67 or more)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402
from gp_cases import random_gps  # noqa: E402
from gp_langevin_cases import np_phi_grad, np_predict_grad  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["RBF", "Matern32", "Matern52"]
H = 1e-5
BAR_MEAN, BAR_VAR, BAR_PHI = 1e-8, 1e-4, 1e-6
LANGEVIN_ENTRY_POINTS = ("cesx_gp_predict_grad", "cesx_gp_langevin_start", "cesx_gp_langevin_propose", "cesx_gp_langevin_accept")


def quotient(f, X, h=H):
    """Central differences of f: (N, p) -> (N,) along every coordinate: (N, p)."""
    out = np.zeros_like(X)
    for q in range(X.shape[1]):
        e = np.zeros(X.shape[1])
        e[q] = h
        out[:, q] = (f(X + e) - f(X - e)) / (2 * h)
    return out


def gp_scales(m, Xq):
    """The sums of absolute terms of one GPR's gradients at Xq, in the GP's own input space."""
    from ces_amd import emulate as em
    L, alpha = m._factor()
    d = m.kern._scaled_diff(m.X, Xq)
    r = np.sqrt((d * d).sum(2))
    beta = np.linalg.solve(L.T, np.linalg.solve(L, m.kern.variance * m.kern.f(r)))
    dk = np.abs((m.kern.variance * m.kern.dfr_over_r(r))[:, :, None] * d / m.kern._ls())
    sm = np.einsum("t,tnq->nq", np.abs(alpha[:, 0]), dk)
    if isinstance(m.mean_function, em.Linear):
        sm = sm + np.abs(m.mean_function.A.reshape(1, -1))
    return sm, 2 * np.einsum("tn,tnq->nq", np.abs(beta), dk)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("scaled", [False, True])
def test_predict_grad_against_central_differences(family, scaled):
    from ces_amd import emulate as em
    rng = np.random.default_rng(7)
    p = 3
    enka = random_gps(rng, p, 3, 40, family, scaled)
    worst = dict(mean=0.0, var=0.0, wrong_var=np.inf, wrong_map=np.inf)
    for m in enka.gpmodels:
        Xq = np.vstack([m.X[:8], 0.7 * rng.standard_normal((12, p))])            # on and off the training points
        mean, var, dm, dv = m.predict_f_grad(Xq)
        m0, v0 = m.predict_f(Xq)
        assert np.array_equal(mean, m0) and np.array_equal(var, v0) and dm.shape == dv.shape == Xq.shape
        sm, sv = gp_scales(m, Xq)
        qm = quotient(lambda X: m.predict_f(X)[0][:, 0], Xq)
        qv = quotient(lambda X: m.predict_f(X)[1][:, 0], Xq)
        worst["mean"] = max(worst["mean"], np.max(np.abs(dm - qm) / sm))
        worst["var"] = max(worst["var"], np.max(np.abs(dv - qv) / sv))
        worst["wrong_var"] = min(worst["wrong_var"], np.max(np.abs(dv / 2 - qv) / sv))        # the factor 2 dropped
        my, vy, dmy, dvy = m.predict_y_grad(Xq)
        assert np.array_equal(dmy, dm) and np.array_equal(dvy, dv) and np.array_equal(vy, var + m.likelihood.variance)
    # predict_gps(grad=True): the unscaled X, through enka.scale
    X = np.vstack([enka.Ustar.T[:8], 0.7 * rng.standard_normal((12, p))])
    gm, gv, dms, dvs = em.predict_gps(enka, X, grad=True)
    g0, v0 = em.predict_gps(enka, X)
    assert np.array_equal(gm, g0) and np.array_equal(gv, v0) and dms.shape == dvs.shape == (3, 20, p)
    _, _, dmr, dvr, sm, sv = np_predict_grad(enka, enka.gpmodels, X)
    for i in range(3):
        qm = quotient(lambda Y: em.predict_gps(enka, Y)[0][i], X)
        qv = quotient(lambda Y: em.predict_gps(enka, Y)[1][i], X)
        worst["mean"] = max(worst["mean"], np.max(np.abs(dms[i] - qm) / sm[i]))
        worst["var"] = max(worst["var"], np.max(np.abs(dvs[i] - qv) / sv[i]))
        assert np.all(np.abs(dms[i] - dmr[i]) <= 1e-9 * sm[i]) and np.all(np.abs(dvs[i] - dvr[i]) <= 1e-9 * sv[i])
        if scaled:                                          # A^T omitted: the gradient in the scaled coordinates
            raw = enka.gpmodels[i].predict_y_grad(np.linalg.solve(enka.scale["cov"], X.T - enka.scale["mean"]).T)[2]
            worst["wrong_map"] = min(worst["wrong_map"], np.max(np.abs(raw - qm) / sm[i]))
    print("[langevin host] %s scaled=%s: %s" % (family, scaled, {k: "%.3g" % v for k, v in worst.items()}))
    assert worst["mean"] <= BAR_MEAN and worst["var"] <= BAR_VAR
    assert worst["wrong_var"] >= 100 * BAR_VAR
    assert not scaled or worst["wrong_map"] >= 100 * BAR_MEAN


PHI_CASES = [("gamma", "diag", "dense"), ("gamma", "dense", "dense"), ("gamma", "dense", "diag"), ("var", None, "dense"),
             ("var", None, "diag"), ("gamma_var", "diag", "dense"), ("gamma_var", "diag", "diag")]


@pytest.mark.parametrize("mode,gamma,prior_kind", PHI_CASES)
def test_grad_phi_against_central_differences(mode, gamma, prior_kind):
    from ces_amd import emulate as em
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    y = np.asarray(a["prob_y"], dtype=np.float64)
    Gamma = None if gamma is None else np.asarray(a["prob_Gamma_" + gamma], dtype=np.float64)
    mu = np.asarray(a["prob_mu"], dtype=np.float64)
    Sig = np.asarray(a["prob_Sigma"], dtype=np.float64)
    Sig = Sig if prior_kind == "dense" else np.diag(np.diag(Sig))
    if prior_kind == "dense":
        assert np.any(Sig != np.diag(np.diag(Sig)))
    rng = np.random.default_rng(3)
    U = np.vstack([enka.Ustar.T[:6], enka.Ustar.mean(axis=1) + 0.3 * rng.standard_normal((10, 2))])      # (N, p)

    def phi(X):
        rows = em.predict_gps(enka, X, grad=True)
        return sample.MCMC.langevin_phi_grad(*rows, X, y, Gamma, mode == "gamma_var", mu, Sig)

    ph, grad = phi(U)
    q = quotient(lambda X: phi(X)[0], U)
    err = np.max(np.abs(grad - q)) / (np.max(np.abs(grad)) + 1)
    # the tests' own restatement agrees with the package's
    m, v, dm, dv, _, _ = np_predict_grad(enka, enka.gpmodels, U)
    pr, gr = np_phi_grad(m, v, dm, dv, U.T, y, mode, Gamma if Gamma is not None else np.eye(4), mu, Sig)
    assert np.allclose(pr, ph, rtol=1e-12, atol=1e-12) and np.allclose(gr, grad, rtol=1e-9, atol=1e-9 * np.max(np.abs(grad)))
    # wrong on purpose: the prior term dropped; in the variance modes the grad var term dropped
    w = np.linalg.solve(Sig, (U - mu).T).T
    wrong = [np.max(np.abs(grad - w - q)) / (np.max(np.abs(grad)) + 1)]
    if mode != "gamma":
        vv = v + (np.diag(Gamma)[:, None] if mode == "gamma_var" else 0.0)
        d = m - y[:, None]
        wrong.append(np.max(np.abs(grad - np.einsum("in,inq->nq", 0.5 * (1 / vv - d * d / vv ** 2), dv) - q)) / (np.max(np.abs(grad)) + 1))
    print("[langevin host] grad phi %s Gamma=%s prior=%s: err %.3g, wrong formulas %s" % (mode, gamma, prior_kind, err, ["%.3g" % x for x in wrong]))
    assert err <= BAR_PHI
    assert min(wrong) >= 100 * BAR_PHI


def test_correction_short_form_equals_the_proposal_densities():
    from ces_amd import sample
    rng = np.random.default_rng(5)
    p, N = 4, 50
    S = np.tril(rng.standard_normal((p, p))) + 2 * np.eye(p)
    gradU, gradP = rng.standard_normal((N, p)), rng.standard_normal((N, p))      # any two gradients: the identity is algebraic
    U, xi = rng.standard_normal((N, p)), rng.standard_normal((N, p))
    gU, gP = gradU @ S, gradP @ S                                                # g = S^T grad phi
    P = U + (xi - 0.5 * gU) @ S.T
    C = S @ S.T

    def logq(to, frm, grad_from):                                               # log N(to; frm - C grad / 2, C) + const
        r = np.linalg.solve(S, (to - frm + 0.5 * grad_from @ C.T).T)
        return -0.5 * (r * r).sum(0)

    long_form = logq(U, P, gradP) - logq(P, U, gradU)
    short = sample.MCMC.langevin_correction(xi, gU, gP)
    assert np.max(np.abs(short - long_form)) <= 1e-10 * (1 + np.max(np.abs(long_form)))
    assert np.max(np.abs(long_form)) > 0.1


def test_host_chain_moves_and_resumes():
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    np.random.seed(2)
    mc.gp_mh(enka, 30, gold_prior(a), delta=0.1, update="langevin", Gamma=a["prob_Gamma_diag"])
    assert mc.samples.shape == (2, 31) and 0.3 < mc.accept <= 1.0 and np.all(np.isfinite(mc.samples))
    mc.gp_mh(enka, 5, gold_prior(a), delta=0.1, update="langevin", Gamma=a["prob_Gamma_diag"])
    assert mc.samples.shape == (2, 36)
    # one chain of the vectorised restatement with the same draws is the same chain
    from gp_langevin_cases import np_chains_langevin
    scales = 0.1 * np.linalg.cholesky(np.cov(enka.Ustar))
    U0 = enka.Ustar.mean(axis=1)[:, None]
    _, _, tr = np_chains_langevin(enka, enka.gpmodels, np.asarray(a["prob_y"]), gold_prior(a), scales, U0, 30, "gamma",
                                  a["prob_Gamma_diag"], True, 2, trace=True)
    np.testing.assert_allclose(mc.samples[:, 1:31], tr[:, :, 0].T, rtol=1e-9, atol=1e-12)


def test_refusals():
    from ces_amd import sample

    class Foreign(object):
        def predict_y(self, X):
            return np.zeros((len(X), 1)), np.ones((len(X), 1))
        predict_f = predict_y

    man, a = load_gold()
    enka = gold_problem(a)
    prior = gold_prior(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    with pytest.raises(UnboundLocalError):                 # pinned by test_emulate_host.py: only 'langevin' is the new option
        mc.gp_mh(enka, 2, prior, update="MALA")
    with pytest.raises(ValueError, match="unknown update"):
        mc.gp_mh(enka, 2, prior, update="MALA", chains=4)
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    for chains in ({}, dict(chains=4)):
        kw = dict(update="langevin", **chains)
        with pytest.raises(ValueError, match="pca_tools"):
            mc.gp_mh(enka, 2, prior, Gamma=a["prob_Gamma_dense"], pca_tools=pca, **kw)
        with pytest.raises(ValueError, match="fused"):
            mc.gp_mh(enka, 2, prior, fused=True, **kw)
        with pytest.raises(ValueError, match="Matern12"):
            mc.gp_mh(gold_problem(a, family="Matern12"), 2, prior, **kw)
        with pytest.raises(ValueError, match="GPR"):
            mc.gp_mh(enka, 2, prior, gpmodels=[Foreign() for _ in range(4)], **kw)
        with pytest.raises(ValueError, match="dense Gamma"):
            mc.gp_mh(enka, 2, prior, Gamma=a["prob_Gamma_dense"], noise_compounded=True, **kw)
    assert not hasattr(mc, "samples")


def test_predict_gps_grad_refusals():
    from ces_amd import emulate as em
    man, a = load_gold()
    enka = gold_problem(a)
    X = enka.Ustar.T[:3]
    with pytest.raises(ValueError, match="pca_tools"):
        em.predict_gps(enka, X, grad=True, pca_tools=dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"]))
    with pytest.raises(ValueError, match="separable"):
        em.predict_gps(enka, X, grad=True, separable=True)
    with pytest.raises(ValueError, match="Matern12"):
        em.predict_gps(gold_problem(a, family="Matern12"), X, grad=True)


def test_model_mh_langevin_is_out_of_scope():
    from ces_amd import sample, utils
    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    model = utils.lineal(np.asarray(a["prob_A"], dtype=np.float64))
    with pytest.raises(ValueError, match="Jacobian"):
        mc.model_mh(model, 2, gold_prior(a), enka, a["prob_Gamma_diag"], chains=4, update="langevin")


def test_abi_10_declared_and_exported():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    assert "#define CESX_MH_LANGEVIN 2" in hdr and engine.MH_KINDS["langevin"] == 2
    for name in LANGEVIN_ENTRY_POINTS:
        assert name + "(" in hdr and name in engine.EXPORTS
    assert "kernels_gpgrad.hip" in build.SOURCES
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10
    for name in LANGEVIN_ENTRY_POINTS:
        assert hasattr(lib, name)
