"""model_mh(update='langevin') on the host: the maps' Jacobians against the reference's values and central differences, the
short acceptance formula against the proposal densities written out, the one-chain host sampler against the vectorised numpy
chains, the invariance of the banana posterior (with the uncorrected sampler as the failing control), the refusals and the
ABI as far as it goes without a GPU.  Cases: tests/map_langevin_cases.py."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _models():
    from ces_amd import utils
    return {"elliptic": utils.elliptic(), "banana": utils.banana(a=1.3, b=0.4)}


def test_elliptic_jacobian_is_the_reference_dG():
    from ces_amd import utils
    g = np.load(os.path.join(GOLD, "maps.npz"))
    mdl = utils.elliptic()
    th = g["el_th1"]
    assert np.array_equal(mdl.jacobian(th), mdl(th, dG=True))
    assert mdl.jacobian(th).shape == (2, 2) and np.allclose(mdl.jacobian(th), g["el_dG1"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_jacobians_against_central_differences(kind):
    """h = 1e-5, within 1e-8 max(1, max|DG|) of the particle's Jacobian (the truncation term h^2 f''' / 6 is 2e-11 relative
    for exp, the rounding term eps |G| / h is 2e-9 at G ~ 80); the (2, 2, J) block is the per-particle calls."""
    mdl = _models()[kind]
    U = mc_.draw_U(kind, 33, np.random.default_rng(3))
    block = mdl.jacobian(U)
    assert block.shape == (2, 2, 33)
    h = 1e-5
    for j in range(U.shape[1]):
        one = mdl.jacobian(U[:, j])
        assert one.shape == (2, 2) and np.array_equal(one, block[:, :, j])
        fd = np.empty((2, 2))
        for q in range(2):
            e = np.zeros(2)
            e[q] = h
            fd[:, q] = (lc.np_map(mdl, (U[:, j] + e)[:, None]) - lc.np_map(mdl, (U[:, j] - e)[:, None]))[:, 0] / (2 * h)
        assert np.max(np.abs(fd - one)) <= 1e-8 * max(1.0, np.max(np.abs(one))), j


def test_short_acceptance_formula():
    """phi(U) - phi(P) + |xi|^2 / 2 - |xi - (g(U) + g(P)) / 2|^2 / 2 equals phi(U) - phi(P) + log q(U | P) - log q(P | U) with
    q(. | x) = N(x - S S^T grad phi(x) / 2, S S^T) written out with S^{-1}: to 1e-10 on 64 random (U, xi)."""
    from ces_amd import sample
    rng = np.random.default_rng(8)
    for kind in ("elliptic", "banana"):
        prob, S = mc_.problem(kind, None), lc.scales(kind)
        Si = np.linalg.inv(S)
        U = mc_.start_ensemble(kind, 64, rng)
        xi = rng.standard_normal((2, 64))
        phi, g = lc.np_phi_g(prob, S, U)
        P = U + S @ (xi - 0.5 * g)
        php, gp = lc.np_phi_g(prob, S, P)
        short = phi - php + sample.MCMC.langevin_correction(xi.T, g.T, gp.T)
        fwd = Si @ (P - (U - 0.5 * S @ g))                 # S^{-1} (P - mean of q(. | U))
        bwd = Si @ (U - (P - 0.5 * S @ gp))
        full = phi - php - 0.5 * (bwd * bwd).sum(axis=0) + 0.5 * (fwd * fwd).sum(axis=0)
        assert np.max(np.abs(short - full)) <= 1e-10 * max(1.0, np.max(np.abs(full))), kind


class _quiet_banana(object):
    """banana without the two normals its host ``__call__`` draws from the global RNG in every call, noise or not (the
    reference's quirk, tests/test_maps_host.py): the same map and Jacobian, draws that the vectorised reference can follow."""

    def __init__(self):
        from ces_amd import utils
        self._m = utils.banana()
        self.type, self.flag_noise, self.model_name = "map", False, "banana"
        self.Gamma, self.jacobian = self._m.Gamma, self._m.jacobian

    def __call__(self, theta):
        return lc.np_map(self._m, np.asarray(theta, dtype=np.float64).reshape(2, 1))[:, 0]


def _host_sampler(kind):
    from ces_amd import calibrate, sample
    model, y, Gamma, mean, cov, _ = mc_.problem(kind, None)
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble(kind, 130, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs = True, y
    return s, enka, stats.multivariate_normal(mean=mean, cov=cov), model, Gamma


@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_host_sampler_is_the_numpy_chain(kind):
    """One host chain equals np_chains_mala with M = 1 under the same seed to 1e-12, ``accept`` included; a second call
    resumes where the first ended (the reference continues with the RNG as it stands)."""
    s, enka, prior, model, Gamma = _host_sampler(kind)
    if kind == "banana":
        model = _quiet_banana()
    n1, n2 = 30, 12
    np.random.seed(21)
    s.model_mh(model, n1, prior, enka, Gamma, delta=lc.DELTA[kind], update="langevin")
    first = s.samples.copy()
    acc1 = s.accept
    s.model_mh(model, n2, prior, enka, Gamma, delta=lc.DELTA[kind], update="langevin")
    assert first.shape == (2, n1 + 1) and s.samples.shape == (2, n1 + n2 + 1)
    assert np.array_equal(s.samples[:, :n1 + 1], first)
    U0 = enka.Ustar.mean(axis=1).reshape(2, 1)
    assert np.array_equal(first[:, 0], U0[:, 0])
    S = lc.scales(kind)
    Ur, a1 = lc.np_chains_mala(kind, S, U0, n1, 21)
    Ur2, a2 = lc.np_chains_mala(kind, S, Ur, n2, None)
    assert np.max(np.abs(first[:, -1] - Ur[:, 0])) <= 1e-12 * (1 + np.max(np.abs(Ur)))
    assert np.max(np.abs(s.samples[:, -1] - Ur2[:, 0])) <= 1e-12 * (1 + np.max(np.abs(Ur2)))
    assert acc1 == pytest.approx(a1[0] / n1, abs=1e-12) and s.accept == pytest.approx(a2[0] / n2, abs=1e-12)
    assert 0 < a1[0] < n1


@pytest.fixture(scope="module")
def quadrature():
    return lc.banana_quadrature()


def test_banana_posterior_is_invariant(quadrature):
    """16 384 chains from the start ensemble, 400 steps in numpy: mean and second central moments within 5 standard errors
    of the quadrature of exp(-phi) (2001^2 points on [-4, 4.5] x [-9, 5]: mean (0.246814, 0.195461), variances (0.237211,
    0.373655)).  Without the correction -- the Langevin proposal under the random walk's test -- the same bound fails on
    the mean and on the variances: the control."""
    mean, var = quadrature
    assert np.allclose(mean, [0.246814, 0.195461], atol=2e-6) and np.allclose(var, [0.237211, 0.373655], atol=2e-6)
    M, steps = 16384, 400
    U0 = mc_.start_ensemble("banana", M, np.random.default_rng(4))
    S = lc.DELTA["banana"] * np.linalg.cholesky(np.cov(U0))
    U, acc = lc.np_chains_mala("banana", S, U0, steps, 3)
    zm, zv = lc.moment_z(U, mean, var)
    rate = acc.sum() / (steps * M)
    print("\n[map langevin host] banana invariance: accept %.4f z mean %s z var %s" % (rate, zm, zv))
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.6 < rate < 0.75
    Uc, _ = lc.np_chains_mala("banana", S, U0, steps, 3, correction=False)
    cm, cv = lc.moment_z(Uc, mean, var)
    print("[map langevin host] without the correction: z mean %s z var %s" % (cm, cv))
    assert np.max(cm) > 5 and np.max(cv) > 5


def test_refusals():
    """No Jacobian: lineal, lineal_log, lorenz63 and a Darcy model raise ValueError("...Jacobian...") with and without chains=4,
    before any engine is created (this runs without a GPU); so does flag_noise=True with its own reason."""
    from ces_amd import darcy, models, utils
    s, enka, prior, _, Gamma = _host_sampler("elliptic")
    refused = [utils.lineal(np.eye(2)), utils.lineal_log(np.eye(2)), models.lorenz63(l_window=1, freq=10), darcy.model(Nmesh=4)]
    for chains in ({}, dict(chains=4)):
        for mdl in refused:
            with pytest.raises(ValueError, match="Jacobian"):
                s.model_mh(mdl, 2, prior, enka, Gamma, update="langevin", **chains)
        for mdl in (utils.elliptic(flag_noise=True), utils.banana(flag_noise=True)):
            with pytest.raises(ValueError, match="flag_noise"):
                s.model_mh(mdl, 2, prior, enka, Gamma, update="langevin", **chains)
    with pytest.raises(ValueError, match="fused"):             # (the host path has one path, Langevin or not)
        s.model_mh(utils.elliptic(), 2, prior, enka, Gamma, update="langevin", fused=True)
    assert not hasattr(s, "samples")


def test_abi_10_with_the_five_entry_points():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    for name in lc.ENTRY_POINTS:
        assert "int %s(" % name in hdr and name in engine.EXPORTS
    assert "kernels_maps.hip" in build.SOURCES
    with open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_maps.hip")) as fh:
        assert "mh_langevin_map_kernel" in fh.read()
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10
    for name in lc.ENTRY_POINTS:
        assert hasattr(lib, name)
