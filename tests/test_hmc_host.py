"""model_mh / gp_mh(update='hmc') on the host: the one-chain samplers against the vectorised numpy chains of
tests/hmc_cases.py, ``leapfrog=1`` against the host ``update='langevin'`` chain, the invariance of the banana posterior (with
the sampler without its kinetic energies as the failing control), the refusals -- each before an engine exists: this file runs
without a GPU -- and the ABI as far as it goes without one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmc_cases as hc  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402
from test_map_langevin_host import _host_sampler, _quiet_banana  # noqa: E402


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_host_model_mh_is_the_numpy_chain(kind, L):
    """One host chain equals np_chains_hmc with M = 1 under the same seed to 1e-12, ``accept`` included; a second call resumes
    where the first ended and scores the resumed state."""
    s, enka, prior, model, Gamma = _host_sampler(kind)
    if kind == "banana":
        model = _quiet_banana()
    n1, n2 = 30, 12
    kw = dict(delta=lc.DELTA[kind], update="hmc", leapfrog=L)
    np.random.seed(21)
    s.model_mh(model, n1, prior, enka, Gamma, **kw)
    first, acc1 = s.samples.copy(), s.accept
    s.model_mh(model, n2, prior, enka, Gamma, **kw)
    assert first.shape == (2, n1 + 1) and s.samples.shape == (2, n1 + n2 + 1)
    assert np.array_equal(s.samples[:, :n1 + 1], first)
    U0 = enka.Ustar.mean(axis=1).reshape(2, 1)
    S = lc.scales(kind)
    Ur, a1 = hc.np_chains_hmc(kind, S, U0, n1, L, 21)
    Ur2, a2 = hc.np_chains_hmc(kind, S, Ur, n2, L, None)
    assert np.max(np.abs(first[:, -1] - Ur[:, 0])) <= 1e-12 * (1 + np.max(np.abs(Ur)))
    assert np.max(np.abs(s.samples[:, -1] - Ur2[:, 0])) <= 1e-12 * (1 + np.max(np.abs(Ur2)))
    assert acc1 == pytest.approx(a1[0] / n1, abs=1e-12) and s.accept == pytest.approx(a2[0] / n2, abs=1e-12)
    assert 0 < a1[0] < n1


def test_default_leapfrog_is_four():
    from ces_amd import sample
    assert sample.MCMC.HMC_LEAPFROG_DEFAULT == 4 and sample.MCMC.HMC_LEAPFROG_MAX == hc.LEAPFROG_MAX
    assert sample.MCMC.HMC_GRADS_MAX == hc.GRADS_MAX
    runs = []
    for kw in ({}, dict(leapfrog=4)):
        s, enka, prior, model, Gamma = _host_sampler("elliptic")
        np.random.seed(3)
        s.model_mh(model, 10, prior, enka, Gamma, delta=lc.DELTA["elliptic"], update="hmc", **kw)
        runs.append(s.samples)
    assert np.array_equal(*runs)


@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var"])
@pytest.mark.parametrize("L", [1, 3])
def test_host_gp_mh_is_the_numpy_chain(L, mode):
    from ces_amd import sample
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    Gamma = None if mode == "var" else a["prob_Gamma_diag"]
    kw = {} if Gamma is None else dict(Gamma=Gamma)
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    n = 20
    np.random.seed(2)
    mc.gp_mh(enka, n, prior, delta=0.1, update="hmc", leapfrog=L, **kw)
    assert mc.samples.shape == (2, n + 1) and np.all(np.isfinite(mc.samples))
    scales = 0.1 * np.linalg.cholesky(np.cov(enka.Ustar))
    U0 = enka.Ustar.mean(axis=1)[:, None]
    Ur, rate = hc.np_chains_hmc_gp(enka, enka.gpmodels, np.asarray(a["prob_y"]), prior, scales, U0, n, L, mode,
                                   Gamma if Gamma is not None else np.eye(4), True, 2)
    np.testing.assert_allclose(mc.samples[:, -1], Ur[:, 0], rtol=1e-9, atol=1e-12)
    assert mc.accept == pytest.approx(rate[0], abs=1e-12) and 0 < mc.accept <= 1


@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_one_leapfrog_is_the_langevin_chain_on_the_host(kind):
    """``leapfrog=1`` and ``update='langevin'`` under one seed: the same states, the same accept (the two differ in the
    rounding of r = (xi - g / 2) - g' / 2 against xi - (g + g') / 2 alone; the proposal is the same expression)."""
    runs = []
    for kw in (dict(update="hmc", leapfrog=1), dict(update="langevin")):
        s, enka, prior, model, Gamma = _host_sampler(kind)
        if kind == "banana":
            model = _quiet_banana()
        np.random.seed(8)
        s.model_mh(model, 40, prior, enka, Gamma, delta=lc.DELTA[kind], **kw)
        runs.append((s.samples, s.accept))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and 0 < runs[0][1] < 1
    # and over 1 025 chains of the vectorised references
    U0 = np.repeat(_host_sampler(kind)[1].Ustar.mean(axis=1)[:, None], 1025, axis=1)
    S = lc.scales(kind)
    Uh, ah = hc.np_chains_hmc(kind, S, U0, 20, 1, 5)
    Ul, al = lc.np_chains_mala(kind, S, U0, 20, 5)
    assert np.array_equal(ah, al) and float(np.max(np.abs(Uh - Ul))) == 0.0


def test_one_leapfrog_is_the_langevin_chain_of_the_emulator():
    from ces_amd import sample
    man, a = load_gold()
    runs = []
    for kw in (dict(update="hmc", leapfrog=1), dict(update="langevin")):
        mc = sample.MCMC()
        mc.mute_bar, mc.y_obs = True, a["prob_y"]
        np.random.seed(2)
        mc.gp_mh(gold_problem(a), 30, gold_prior(a), delta=0.1, Gamma=a["prob_Gamma_diag"], **kw)
        runs.append((mc.samples, mc.accept))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


@pytest.fixture(scope="module")
def quadrature():
    return lc.banana_quadrature()


def test_banana_posterior_is_invariant(quadrature):
    """16 384 chains from the start ensemble, 400 steps of L = 4 in numpy at ``scales('banana')``: mean and second central moments
    within 5 standard errors of the quadrature of exp(-phi), accept in (0.55, 0.67) (0.607 and a worst z of 2.1 for seeds 5,
    6, 7).  Without the kinetic energies in the test the same bound fails (z = 21 .. 76): the control."""
    mean, var = quadrature
    M, steps, L = 16384, 400, 4
    U0 = mc_.start_ensemble("banana", M, np.random.default_rng(4))
    S = lc.scales("banana")                                # (of the 130-particle ensemble, as the samplers' cases form it)
    U, acc = hc.np_chains_hmc("banana", S, U0, steps, L, 5)
    zm, zv = lc.moment_z(U, mean, var)
    rate = acc.sum() / (steps * M)
    print("\n[hmc host] banana invariance: accept %.4f z mean %s z var %s" % (rate, zm, zv))
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.55 < rate < 0.67
    Uc, _ = hc.np_chains_hmc("banana", S, U0, steps, L, 5, kinetic=False)
    cm, cv = lc.moment_z(Uc, mean, var)
    print("[hmc host] without the kinetic energies: z mean %s z var %s" % (cm, cv))
    assert max(np.max(cm), np.max(cv)) > 5


def test_refusals():
    """Everything update='langevin' refuses, the linear maps with and without enable_gradient(), a leapfrog that is no
    integer in [1, 64] and leapfrog= with another update: ValueError with and without chains=4, before any engine is created."""
    from ces_amd import darcy, models, sample, utils
    s, enka, prior, _, Gamma = _host_sampler("elliptic")
    lin, linlog = utils.lineal(np.eye(2)), utils.lineal_log(np.eye(2))
    lin_g, linlog_g = utils.lineal(np.eye(2)), utils.lineal_log(np.eye(2))
    lin_g.enable_gradient()
    linlog_g.enable_gradient()
    for chains in ({}, dict(chains=4)):
        for mdl in (lin, linlog, lin_g, linlog_g):
            with pytest.raises(ValueError, match="follow-up"):
                s.model_mh(mdl, 2, prior, enka, Gamma, update="hmc", **chains)
        for mdl in (models.lorenz63(l_window=1, freq=10), darcy.model(Nmesh=4)):
            with pytest.raises(ValueError, match="Jacobian") as exc:
                s.model_mh(mdl, 2, prior, enka, Gamma, update="hmc", **chains)
            assert "update='hmc'" in str(exc.value)
        for mdl in (utils.elliptic(flag_noise=True), utils.banana(flag_noise=True)):
            with pytest.raises(ValueError, match="flag_noise"):
                s.model_mh(mdl, 2, prior, enka, Gamma, update="hmc", **chains)
        with pytest.raises(ValueError, match="mean and .cov"):
            s.model_mh(utils.elliptic(), 2, object(), enka, Gamma, update="hmc", **chains)
        for bad in (0, 65, -1, 2.0, "4", True, [4]):
            with pytest.raises(ValueError, match="leapfrog must be an integer"):
                s.model_mh(utils.elliptic(), 2, prior, enka, Gamma, update="hmc", leapfrog=bad, **chains)
        for update in (None, "pCN", "langevin"):
            with pytest.raises(ValueError, match="leapfrog=4 counts"):
                s.model_mh(utils.elliptic(), 2, prior, enka, Gamma, update=update, leapfrog=4, **chains)
    with pytest.raises(ValueError, match="fused"):             # (the host path has one path)
        s.model_mh(utils.elliptic(), 2, prior, enka, Gamma, update="hmc", fused=True)
    with pytest.raises(ValueError, match="summary"):
        s.model_mh(utils.elliptic(), 2, prior, enka, Gamma, update="hmc", summary=True)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")

    # the emulator
    class Foreign(object):
        def predict_y(self, X):
            return np.zeros((len(X), 1)), np.ones((len(X), 1))
        predict_f = predict_y

    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    for chains in ({}, dict(chains=4)):
        kw = dict(update="hmc", **chains)
        with pytest.raises(ValueError, match="pca_tools") as exc:
            mc.gp_mh(enka, 2, prior, Gamma=a["prob_Gamma_dense"], pca_tools=pca, **kw)
        assert "update='hmc'" in str(exc.value)
        with pytest.raises(ValueError, match="separable"):
            mc.gp_mh(enka, 2, prior, separable=True, **kw)
        with pytest.raises(ValueError, match="fused"):
            mc.gp_mh(enka, 2, prior, fused=True, **kw)
        with pytest.raises(ValueError, match="Matern12"):
            mc.gp_mh(gold_problem(a, family="Matern12"), 2, prior, **kw)
        with pytest.raises(ValueError, match="GPR"):
            mc.gp_mh(enka, 2, prior, gpmodels=[Foreign() for _ in range(4)], **kw)
        with pytest.raises(ValueError, match="dense Gamma"):
            mc.gp_mh(enka, 2, prior, Gamma=a["prob_Gamma_dense"], noise_compounded=True, **kw)
        for bad in (0, 65, 1.5, False):
            with pytest.raises(ValueError, match="leapfrog must be an integer"):
                mc.gp_mh(enka, 2, prior, leapfrog=bad, **kw)
        for update in (None, "pCN", "langevin"):
            with pytest.raises(ValueError, match="leapfrog=2 counts"):
                mc.gp_mh(enka, 2, prior, update=update, leapfrog=2, **chains)
    assert not hasattr(mc, "samples") and not hasattr(mc, "_mh_eng")


def test_abi_10_with_the_six_entry_points():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    assert "#define CESX_HMC_LEAPFROG_MAX %d" % hc.LEAPFROG_MAX in hdr and "#define CESX_HMC_LAUNCH_GRADS_MAX %d" % hc.GRADS_MAX in hdr
    for name in hc.ENTRY_POINTS:
        assert "int %s(" % name in hdr and name in engine.EXPORTS
    assert "kernels_hmc.hip" in build.SOURCES and any(h.endswith("lv_score.h") for h in build.HEADERS)
    with open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_maps.hip")) as fh:
        assert "mh_hmc_map_kernel" in fh.read()
    assert engine.MH_KINDS["hmc"] == engine.MH_KINDS["langevin"]       # no proposal kind of its own
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10
    for name in hc.ENTRY_POINTS:
        assert hasattr(lib, name)
