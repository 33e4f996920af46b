"""model_mh(update='langevin') for the linear maps on the host: ``enable_gradient()`` and what it offers, the one-chain host
sampler against the vectorised numpy chains, the Jacobians against central differences, the refusals without the opt-in, the
invariance of the exact Gaussian posterior (with the uncorrected sampler as the failing control), the bound of g against its
mutants, the steps of the cases, and the ABI as far as it goes without a GPU.  Cases: tests/lineal_langevin_cases.py."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lineal_langevin_cases as lc  # noqa: E402


def _host_sampler(prob):
    from ces_amd import calibrate, sample
    enka = calibrate.enka(prob["p"], prob["n"], 130)
    enka.Ustar = prob["ens"]
    s = sample.MCMC()
    s.mute_bar, s.y_obs = True, prob["y"]
    return s, enka, stats.multivariate_normal(mean=prob["mu"], cov=prob["Sigma"])


@pytest.mark.parametrize("name, forms", [("lineal-5x3", (True, True)), ("lineal-17x33", (False, True)), ("log-5x3", (True, False)),
                                         ("log-17x33", (False, False))])
def test_host_sampler_is_the_numpy_chain(name, forms):
    """After enable_gradient() one host chain equals np_chains_mala_lineal with M = 1 under the same seed to 1e-10, ``accept``
    included; a second call resumes where the first ended.  (On the parent commit lineal has no enable_gradient.)"""
    prob = lc.problem(name, *forms)
    model = lc.model_of(prob)
    s, enka, prior = _host_sampler(prob)
    p, n1, n2 = prob["p"], 30, 12
    np.random.seed(21)
    s.model_mh(model, n1, prior, enka, prob["Gamma"], delta=prob["delta"], update="langevin")
    first, acc1 = s.samples.copy(), s.accept
    s.model_mh(model, n2, prior, enka, prob["Gamma"], delta=prob["delta"], update="langevin")
    assert first.shape == (p, n1 + 1) and s.samples.shape == (p, n1 + n2 + 1)
    assert np.array_equal(s.samples[:, :n1 + 1], first)
    U0 = enka.Ustar.mean(axis=1).reshape(p, 1)
    S = lc.scales(prob)
    Ur, a1 = lc.np_chains_mala_lineal(prob, S, U0, n1, 21)
    Ur2, a2 = lc.np_chains_mala_lineal(prob, S, Ur, n2, None)
    assert np.max(np.abs(first[:, -1] - Ur[:, 0])) <= 1e-10 * (1 + np.max(np.abs(Ur)))
    assert np.max(np.abs(s.samples[:, -1] - Ur2[:, 0])) <= 1e-10 * (1 + np.max(np.abs(Ur2)))
    assert acc1 == pytest.approx(a1[0] / n1, abs=1e-12) and s.accept == pytest.approx(a2[0] / n2, abs=1e-12)
    assert 0 < a1[0] < n1


@pytest.mark.parametrize("name", ["lineal-5x3", "lineal-17x33", "log-5x3", "log-17x33"])
def test_jacobian_against_central_differences(name):
    """h = 1e-5: within 1e-6 max|DG| of the central difference of ``__call__`` (truncation h^2 / 6, rounding eps |G| / h)."""
    prob = lc.problem(name, False, False)
    model = lc.model_of(prob)
    p, n, h = prob["p"], prob["n"], 1e-5
    for j in range(3):
        u = prob["ens"][:, j]
        DG = model.jacobian(u)
        assert DG.shape == (n, p)
        fd = np.empty((n, p))
        for q in range(p):
            e = np.zeros(p)
            e[q] = h
            fd[:, q] = (np.asarray(model(u + e)) - np.asarray(model(u - e))) / (2 * h)
        assert np.max(np.abs(fd - DG)) <= 1e-6 * np.max(np.abs(DG)), (name, j)
    want = prob["A"] if prob["kind"] == "lineal" else prob["A"] * np.exp(u)[None, :]
    assert np.array_equal(DG, want)


def test_the_gradient_is_opt_in():
    """Without enable_gradient() neither attribute exists and the refusal is the old one, now naming the opt-in; with it a
    noisy map keeps its own refusal and fused=True the chain kernel's."""
    from ces_amd import utils
    prob = lc.problem("lineal-5x3", False, False)
    s, enka, prior = _host_sampler(prob)
    for mdl in (utils.lineal(prob["A"], prob["b"]), utils.lineal_log(prob["A"])):
        assert not hasattr(mdl, "jacobian") and not hasattr(mdl, "langevin_device")
        for chains in ({}, dict(chains=4)):
            with pytest.raises(ValueError, match="Jacobian") as exc:
                s.model_mh(mdl, 2, prior, enka, prob["Gamma"], update="langevin", **chains)
            assert "enable_gradient()" in str(exc.value)
        assert mdl.enable_gradient() is mdl and hasattr(mdl, "jacobian") and hasattr(mdl, "langevin_device")
    for cls in (lambda: utils.lineal(prob["A"], prob["b"], flag_noise=True), lambda: utils.lineal_log(prob["A"], flag_noise=True)):
        for chains in ({}, dict(chains=4)):
            with pytest.raises(ValueError, match="flag_noise"):
                s.model_mh(cls().enable_gradient(), 2, prior, enka, prob["Gamma"], update="langevin", **chains)
    with pytest.raises(ValueError, match="no fused chain kernel"):
        s.model_mh(lc.model_of(prob), 2, prior, enka, prob["Gamma"], update="langevin", chains=4, fused=True)
    assert not hasattr(s, "samples")


def test_gaussian_posterior_is_invariant():
    """lineal, p = 5: 4 096 numpy chains started from exact posterior draws keep, after 200 steps, mean and variances within 5
    standard errors of m and diag C.  Without the correction -- the Langevin proposal under the random walk's test -- some z
    exceeds 5: the control."""
    prob = lc.problem("lineal-5x3", False, False)
    M, steps = 4096, 200
    S, U0 = lc.scales(prob), lc.exact_draws(prob, M, 11)
    U, acc = lc.np_chains_mala_lineal(prob, S, U0, steps, 3)
    zm, zv = lc.moment_z(U, prob["m"], np.diag(prob["C"]))
    rate = acc.sum() / (steps * M)
    print("\n[lineal langevin host] invariance: accept %.4f z mean %s z var %s" % (rate, zm, zv))
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.5 < rate < 0.95
    Uc, _ = lc.np_chains_mala_lineal(prob, S, U0, steps, 3, correction=False)
    cm, cv = lc.moment_z(Uc, prob["m"], np.diag(prob["C"]))
    print("[lineal langevin host] without the correction: z mean %s z var %s" % (cm, cv))
    assert max(np.max(cm), np.max(cv)) > 5


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_bound_of_g_rejects_the_mutants(name):
    """The fp32 bound c 2^-24 mag (the wider of the two) is exceeded somewhere by a g without the -A^T Gamma^{-1} y bias,
    without the prior term, with S in place of S^T and (lineal_log) without the exp factor, for every form of Gamma and Sigma."""
    for forms in lc.FORMS:
        prob = lc.problem(name, *forms)
        S, U = lc.scales(prob), prob["ens"][:, :65]
        _, g = lc.np_phi_g(prob, S, U)
        bound = lc.g_bound(prob, S, U, "float32")
        assert np.all(bound > 0)
        for mutant in lc.MUTANTS:
            if mutant == "exp_missing" and prob["kind"] != "lineal_log":
                continue
            _, gm = lc.np_phi_g(prob, S, U, mutant=mutant)
            assert np.any(np.abs(gm - g) > bound), (name, forms, mutant)


def test_steps_accept_between_half_and_095():
    """The step of every case: the numpy accept rate over 20 steps of 1 025 chains from the ensemble mean lies in (0.5, 0.95)."""
    for name in lc.CASES:
        for forms in lc.FORMS:
            prob = lc.problem(name, *forms)
            U0 = np.repeat(prob["ens"].mean(axis=1)[:, None], 1025, axis=1)
            _, acc = lc.np_chains_mala_lineal(prob, lc.scales(prob), U0, 20, 5)
            rate = acc.sum() / (20 * 1025)
            print("[lineal langevin host] %s dense Gamma %d dense Sigma %d: accept %.3f" % ((name,) + forms + (rate,)))
            assert 0.5 < rate < 0.95, (name, forms, rate)


def test_abi_10_with_the_five_entry_points():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    for name in lc.ENTRY_POINTS:
        assert "int %s(" % name in hdr and name in engine.EXPORTS
    assert "kernels_lvlin.hip" in build.SOURCES
    with open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_lvlin.hip")) as fh:
        assert "lvlin_accept_kernel" in fh.read()
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10
    for name in lc.ENTRY_POINTS:
        assert hasattr(lib, name)
