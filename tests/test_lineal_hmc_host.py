"""model_mh(update='hmc', adapt=) for the linear maps without a GPU: the one-chain host sampler on the models marked by
``enable_gradient(leapfrog=True)`` against the numpy chains of tests/lineal_hmc_cases.py, the invariance of the reference itself
with its failing control, the refusals, and the ABI as far as it goes without a device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapt_cases as ac  # noqa: E402
import hmc_cases as hc  # noqa: E402
import lineal_hmc_cases as hl  # noqa: E402
import lineal_langevin_cases as lc  # noqa: E402

CASES = [("lineal-17x33", (True, True)), ("log-5x3", (False, True))]


def _close(a, b, cap=1e-9):
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= cap * (1 + np.abs(np.asarray(b)))))


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("name, forms", CASES)
def test_host_chain_against_numpy(name, forms, L):
    """20 steps of the host sampler under one seed against ``_hmc_steps`` at M = 1: every state within 1e-9 (1 + |U|), the
    accept rate within 1e-12; ``leapfrog=1`` gives the states of the host Langevin run."""
    prob = lc.problem(name, *forms)
    steps = 20
    s, enka, prior = hl.sampler(prob)
    np.random.seed(13)
    s.model_mh(hl.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], update="hmc", leapfrog=L)
    U0 = enka.Ustar.mean(axis=1)[:, None]
    keep = []
    _, acc = hl.np_chains(prob, lc.scales(prob), U0, steps, L, 13, keep=keep)
    assert s.samples.shape == (prob["p"], steps + 1)
    assert _close(s.samples[:, 1:], np.array(keep)[:, :, 0].T)
    assert abs(s.accept - acc[0] / steps) <= 1e-12 and 0 < s.accept <= 1
    if L == 1:
        t, enka, prior = hl.sampler(prob)
        np.random.seed(13)
        t.model_mh(lc.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], update="langevin")
        assert _close(s.samples, t.samples) and abs(s.accept - t.accept) <= 1e-12


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("name, forms", CASES)
def test_host_adapt_against_numpy(name, forms, L):
    """``adapt=15`` of 40 steps from a step 3 x too long under one seed against ``np_adapt`` with M = 1: the states, the
    histories and the multiplier within 1e-9; ``self.adapt`` is filled; the 25 steps behind run at delta * multiplier."""
    prob = lc.problem(name, *forms)
    update = "langevin" if L == 1 else "hmc"
    kw = dict(update=update) if L == 1 else dict(update=update, leapfrog=L)
    A, n, delta = 15, 40, 3.0 * prob["delta"]
    s, enka, prior = hl.sampler(prob)
    np.random.seed(21)
    s.model_mh(hl.model_of(prob), n, prior, enka, prob["Gamma"], delta=delta, adapt=A, **kw)
    U0 = enka.Ustar.mean(axis=1)[:, None]
    S = hl.scales(prob, 3.0)
    np.random.seed(21)
    states, hist, mult, _ = ac.np_adapt(hl.score_of(prob, S), S, U0, A, L, ac.TARGET[update])
    S2 = (delta * mult) * np.linalg.cholesky(np.cov(enka.Ustar))
    after = []
    _, acc = hc._hmc_steps(hl.score_of(prob, S2), S2, states[-1], n - A, L, keep=after)
    assert s.samples.shape == (prob["p"], 1 + n)
    assert _close(s.samples[:, 1:A + 1], states[:, :, 0].T) and _close(s.samples[:, A + 1:], np.array(after)[:, :, 0].T)
    ad = s.adapt
    assert ad["steps"] == A and ad["target"] == ac.TARGET[update] and ad["delta"] == float(delta) * ad["multiplier"]
    assert _close(ad["multiplier_history"], hist[:, 0]) and _close(ad["accept_history"], hist[:, 1]) and _close(ad["multiplier"], mult)
    assert ad["multiplier"] != 1.0 and ad["multiplier_history"][0] == 1.0
    assert s.accept == pytest.approx(acc[0] / (n - A), abs=1e-12)


def test_the_reference_leaves_the_gaussian_posterior_invariant():
    """16 384 exact posterior draws of lineal-5x3, L = 4, 100 steps of the numpy chains: the z of the mean and of the variances
    stay within 5; without the kinetic terms in the test (a wrong sampler) the largest is above 5."""
    prob = lc.problem("lineal-5x3", False, False)
    S = lc.scales(prob)
    U0 = lc.exact_draws(prob, 16384, 11)
    U, acc = hl.np_chains(prob, S, U0, 100, 4, 3)
    zm, zv = lc.moment_z(U, prob["m"], np.diag(prob["C"]))
    print("\n[lineal hmc host] invariance: accept %.4f z mean %s z var %s" % (acc.sum() / (100 * 16384), zm, zv))
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    Ub, _ = hl.np_chains(prob, S, U0, 100, 4, 3, kinetic=False)
    zmb, zvb = lc.moment_z(Ub, prob["m"], np.diag(prob["C"]))
    assert max(zmb.max(), zvb.max()) > 5, (zmb, zvb)


def test_refusals():
    """The marked models still refuse what update='langevin' refuses and fused=True; unmarked instances are refused as before."""
    from scipy import stats
    from ces_amd import utils
    prob = lc.problem("lineal-5x3", False, False)
    s, enka, prior = hl.sampler(prob)
    Gamma, A = prob["Gamma"], prob["A"]
    for chains in ({}, dict(chains=4)):
        for kw in (dict(update="hmc", leapfrog=2), dict(update="langevin", adapt=5), dict(update="hmc", adapt=5)):
            for mdl in (utils.lineal(A, flag_noise=True), utils.lineal_log(A, flag_noise=True)):
                with pytest.raises(ValueError, match="flag_noise"):
                    s.model_mh(mdl.enable_gradient(leapfrog=True), 20, prior, enka, Gamma, **kw, **chains)
            with pytest.raises(ValueError, match="mean and .cov"):
                s.model_mh(hl.model_of(prob), 20, stats.norm(), enka, Gamma, **kw, **chains)
            # unmarked: without enable_gradient() and with it as it is called today
            for mdl in (lc.model_of(prob), hl.model_of(prob).enable_gradient()):
                with pytest.raises(ValueError, match="follow-up"):
                    s.model_mh(mdl, 20, prior, enka, Gamma, **kw, **chains)
            # a plain lineal has no gradient at all: update='langevin' says so first, update='hmc' refuses the linear map
            with pytest.raises(ValueError, match="no Jacobian" if kw["update"] == "langevin" else "follow-up"):
                s.model_mh(lc.model_of(prob, gradient=False), 20, prior, enka, Gamma, **kw, **chains)
        with pytest.raises(ValueError, match="GEMM-form leapfrog"):
            s.model_mh(lc.model_of(prob), 20, prior, enka, Gamma, update="hmc", **chains)
        with pytest.raises(ValueError, match="kernels_lvlin.hip"):
            s.model_mh(lc.model_of(prob), 20, prior, enka, Gamma, update="langevin", adapt=5, **chains)
    with pytest.raises(ValueError, match="fused=True"):
        s.model_mh(hl.model_of(prob), 20, prior, enka, Gamma, update="hmc", leapfrog=2, chains=4, fused=True)
    with pytest.raises(ValueError, match="leapfrog must be False or True"):
        lc.model_of(prob, gradient=False).enable_gradient(leapfrog=2)
    mdl = hl.model_of(prob)
    assert mdl.leapfrog_device is True and not hasattr(mdl.enable_gradient(), "leapfrog_device")
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng") and not hasattr(s, "adapt")


def test_abi_10_with_the_hmc_lineal_entry_points():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    for name in hl.ENTRY_POINTS:
        assert "int %s(" % name in hdr and name in engine.EXPORTS
    assert "kernels_hmclin.hip" in build.SOURCES
    with open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_hmclin.hip")) as fh:
        src = fh.read()
    for k in ("hl_kick_kernel", "hl_accept_kernel"):
        assert k in src
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10
    for name in hl.ENTRY_POINTS:
        assert hasattr(lib, name)
    for name in ("mh_hmc_lineal_begin", "mh_hmc_lineal_leap", "mh_hmc_lineal_accept"):
        assert hasattr(engine.Engine, name)
