"""model_mh / gp_mh(adapt=) without a GPU: the numpy reference of tests/adapt_cases.py converges on the cases the device
tests use (conditions on the inputs), the one-chain host samplers equal it at M = 1, every refusal is raised before an engine
exists, and the ABI as far as it goes without a device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapt_cases as ac  # noqa: E402
import hmc_cases as hc  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402
from test_map_langevin_host import _host_sampler, _quiet_banana  # noqa: E402

FACTORS = {"long": 8.0, "short": 1.0 / 16.0}               # delta = factor * lc.DELTA: a step 8 x too long, one 16 x too short


@pytest.mark.parametrize("which", ["long", "short"])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_the_reference_converges(kind, L, which):
    """512 chains from the start ensemble, A = 100: without adaptation the step accepts below 0.05 (8 x) or above 0.95
    (1 / 16 x); at delta * multiplier the next 60 steps accept within 0.025 of the target.  numpy alone."""
    from ces_amd import sample
    f = FACTORS[which]
    target = ac.TARGET["langevin" if L == 1 else "hmc"]
    assert sample.ADAPT_TARGETS == ac.TARGET and (sample.ADAPT_GAIN, sample.ADAPT_KAPPA) == (ac.GAIN, ac.KAPPA)      # the package's defaults are the ones that converge here
    U0 = mc_.start_ensemble(kind, 512, np.random.default_rng(4))
    S = ac.scales(kind, f)
    score = ac.map_score(kind, S)
    np.random.seed(11)
    raw = ac.np_accept_rate(score, S, U0, 60, L)
    assert raw < 0.05 if which == "long" else raw > 0.95, raw
    np.random.seed(12)
    states, hist, mult, _ = ac.np_adapt(score, S, U0, 100, L, target)
    S2 = ac.scales(kind, f * mult)
    rate = ac.np_accept_rate(ac.map_score(kind, S2), S2, states[-1], 60, L)
    print("\n[adapt host] %s L=%d %s: raw %.3f multiplier %.4f accept %.4f target %.3f" % (kind, L, which, raw, mult, rate, target))
    assert abs(rate - target) <= 0.025, (rate, target)
    assert hist.shape == (100, 2) and hist[0, 0] == 1.0 and np.all((hist[:, 1] >= 0) & (hist[:, 1] <= 1))


def _close(a, b):
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 1e-9 * (1 + np.abs(np.asarray(b)))))


def _check_adapt(s, delta, A, L, update, states, hist, mult, after):
    assert s.samples.shape == (states.shape[1], 1 + A + after.shape[0])
    assert _close(s.samples[:, 1:A + 1], states[:, :, 0].T)
    assert _close(s.samples[:, A + 1:], after[:, :, 0].T)
    ad = s.adapt
    assert sorted(ad) == ["accept_history", "delta", "multiplier", "multiplier_history", "steps", "target"]
    assert ad["steps"] == A and ad["target"] == ac.TARGET[update]
    assert ad["accept_history"].shape == ad["multiplier_history"].shape == (A,)
    assert _close(ad["multiplier_history"], hist[:, 0]) and _close(ad["accept_history"], hist[:, 1]) and _close(ad["multiplier"], mult)
    assert ad["delta"] == float(delta) * ad["multiplier"]
    assert ad["multiplier"] != 1.0 and ad["multiplier_history"][0] == 1.0


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_host_model_mh_is_the_reference_at_one_chain(kind, L):
    """``adapt=15`` of 40 steps under one seed: the states of every step, the histories and the multiplier within
    1e-9 (1 + |x|); ``delta == delta_in * multiplier`` exactly; ``accept`` covers the 25 steps at the frozen step.  L = 1 is
    ``update='langevin'`` with its own target."""
    s, enka, prior, model, Gamma = _host_sampler(kind)
    if kind == "banana":
        model = _quiet_banana()
    update = "langevin" if L == 1 else "hmc"
    kw = dict(update=update) if L == 1 else dict(update=update, leapfrog=L)
    A, n, delta = 15, 40, 3.0 * lc.DELTA[kind]
    np.random.seed(21)
    s.model_mh(model, n, prior, enka, Gamma, delta=delta, adapt=A, **kw)
    U0 = enka.Ustar.mean(axis=1).reshape(2, 1)
    S = ac.scales(kind, 3.0)
    np.random.seed(21)
    states, hist, mult, _ = ac.np_adapt(ac.map_score(kind, S), S, U0, A, L, ac.TARGET[update])
    S2 = (delta * mult) * np.linalg.cholesky(np.cov(enka.Ustar))
    after = []
    _, acc = hc._hmc_steps(ac.map_score(kind, S2), S2, states[-1], n - A, L, keep=after)
    _check_adapt(s, delta, A, L, update, states, hist, mult, np.array(after))
    assert s.accept == pytest.approx(acc[0] / (n - A), abs=1e-12)
    s.model_mh(model, 5, prior, enka, Gamma, delta=delta, **kw)      # a call without adapt= removes self.adapt
    assert not hasattr(s, "adapt") and s.samples.shape == (2, n + 6)


@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var"])
@pytest.mark.parametrize("L", [1, 3])
def test_host_gp_mh_is_the_reference_at_one_chain(L, mode):
    from ces_amd import sample
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    Gamma = None if mode == "var" else a["prob_Gamma_diag"]
    kw = {} if Gamma is None else dict(Gamma=Gamma)
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    update = "langevin" if L == 1 else "hmc"
    kw.update(dict(update=update) if L == 1 else dict(update=update, leapfrog=L))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    A, n, delta = 10, 24, 0.3
    np.random.seed(2)
    mc.gp_mh(enka, n, prior, delta=delta, adapt=dict(steps=A), **kw)
    C = np.linalg.cholesky(np.cov(enka.Ustar))
    G = Gamma if Gamma is not None else np.eye(4)
    y, U0 = np.asarray(a["prob_y"]), enka.Ustar.mean(axis=1)[:, None]
    np.random.seed(2)
    states, hist, mult, _ = ac.np_adapt(ac.gp_score(enka, enka.gpmodels, y, prior, delta * C, mode, G), delta * C, U0, A, L,
                                        ac.TARGET[update])
    S2 = (delta * mult) * C
    after = []
    _, acc = hc._hmc_steps(ac.gp_score(enka, enka.gpmodels, y, prior, S2, mode, G), S2, states[-1], n - A, L, keep=after)
    _check_adapt(mc, delta, A, L, update, states, hist, mult, np.array(after))
    assert mc.accept == pytest.approx(acc[0] / (n - A), abs=1e-12)


def test_adapt_spec():
    from ces_amd import sample
    assert sample.adapt_spec(None, "hmc") is None and sample.adapt_spec(False, None) is None
    assert sample.adapt_spec(True, "hmc") == dict(steps=100, target=0.651, gain=2.0, kappa=0.75)
    assert sample.adapt_spec(7, "langevin") == dict(steps=7, target=0.574, gain=2.0, kappa=0.75)
    assert sample.adapt_spec(dict(steps=3, target=0.8, gain=1, kappa=1.0), "hmc") == dict(steps=3, target=0.8, gain=1.0, kappa=1.0)
    assert sample.ADAPT_STEPS_MAX == ac.STEPS_MAX and sample.ADAPT_TARGETS == ac.TARGET
    for bad in (dict(step=3), dict(steps=True), dict(steps=2.0), dict(steps=0), dict(steps=65537), 0, -1, 65537, 2.5, "10",
                dict(target=0.0), dict(target=1.0), dict(gain=0.0), dict(gain=-1), dict(kappa=0.5), dict(kappa=1.5),
                dict(target="x"), dict(gain=True)):
        with pytest.raises(ValueError, match="adapt"):
            sample.adapt_spec(bad, "hmc")


def test_refusals():
    """What ``adapt=`` does not go with, with and without chains=4: a ValueError before any engine is created; what
    ``update=`` refuses stays refused with its own message."""
    from ces_amd import sample, utils
    s, enka, prior, _, Gamma = _host_sampler("elliptic")
    ell = utils.elliptic()
    lin_g, linlog_g = utils.lineal(np.eye(2)), utils.lineal_log(np.eye(2))
    lin_g.enable_gradient()
    linlog_g.enable_gradient()
    for chains in ({}, dict(chains=4)):
        for update in (None, "pCN"):                      # the random walk's and pCN's proposals are update launches
            with pytest.raises(ValueError, match="update launch"):
                s.model_mh(ell, 20, prior, enka, Gamma, update=update, adapt=5, **chains)
        for mdl in (lin_g, linlog_g):                     # the GEMM-form Langevin step
            with pytest.raises(ValueError, match="kernels_lvlin.hip") as exc:
                s.model_mh(mdl, 20, prior, enka, Gamma, update="langevin", adapt=5, **chains)
            assert "follow-up" in str(exc.value)
        for kw in (dict(update="langevin"), dict(update="hmc", leapfrog=2)):
            for A in (20, 21, dict(steps=30)):            # A >= n_mcmc
                with pytest.raises(ValueError, match="leaves none"):
                    s.model_mh(ell, 20, prior, enka, Gamma, adapt=A, **kw, **chains)
            for bad in (dict(steps=True), 2.5, dict(steps=0), dict(steps=65537), dict(stride=2), "3"):
                with pytest.raises(ValueError, match="adapt"):
                    s.model_mh(ell, 20, prior, enka, Gamma, adapt=bad, **kw, **chains)
        # what update= refuses stays refused, with its own message
        with pytest.raises(ValueError, match="flag_noise"):
            s.model_mh(utils.elliptic(flag_noise=True), 20, prior, enka, Gamma, update="langevin", adapt=5, **chains)
        with pytest.raises(ValueError, match="follow-up") as exc:
            s.model_mh(lin_g, 20, prior, enka, Gamma, update="hmc", adapt=5, **chains)
        assert "GEMM-form leapfrog" in str(exc.value)
    s.trace_stride = 3
    with pytest.raises(ValueError, match="trace_stride 3"):
        s.model_mh(ell, 20, prior, enka, Gamma, update="hmc", adapt=4, chains=4)
    s.trace_stride = 1
    for burn in ({}, dict(burn=4), dict(burn=0)):
        with pytest.raises(ValueError, match="burn >= 5"):
            s.model_mh(ell, 40, prior, enka, Gamma, update="hmc", adapt=5, chains=4, summary=True, **burn)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng") and not hasattr(s, "adapt")

    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    for chains in ({}, dict(chains=4)):
        for update in (None, "pCN"):
            with pytest.raises(ValueError, match="update launch"):
                mc.gp_mh(enka, 20, prior, update=update, adapt=True, **chains)
        with pytest.raises(ValueError, match="leaves none"):
            mc.gp_mh(enka, 100, prior, update="langevin", adapt=True, **chains)
        with pytest.raises(ValueError, match="unknown key"):
            mc.gp_mh(enka, 20, prior, update="hmc", adapt=dict(steps=4, rate=0.5), **chains)
        with pytest.raises(ValueError, match="pca_tools"):
            mc.gp_mh(enka, 20, prior, update="langevin", adapt=5, Gamma=a["prob_Gamma_dense"], pca_tools=pca, **chains)
    mc.trace_stride = 4
    with pytest.raises(ValueError, match="trace_stride 4"):
        mc.gp_mh(enka, 20, prior, update="langevin", adapt=6, chains=4)
    mc.trace_stride = 1
    with pytest.raises(ValueError, match="burn >= 8"):
        mc.gp_mh(enka, 40, prior, update="langevin", adapt=8, chains=4, summary=True, burn=7)
    assert not hasattr(mc, "samples") and not hasattr(mc, "_mh_eng") and not hasattr(mc, "adapt")


def test_abi_10_with_the_adapt_entry_points():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    assert "#define CESX_ADAPT_STEPS_MAX %d" % ac.STEPS_MAX in hdr
    for name in ac.ENTRY_POINTS:
        assert "int %s(" % name in hdr and name in engine.EXPORTS
    assert "kernels_adapt.hip" in build.SOURCES
    with open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_adapt.hip")) as fh:
        assert "ad_update_kernel" in fh.read()
    with open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_hmc.hip")) as fh:
        src = fh.read()
    for k in ("hm_begin_kernel", "hm_leap_kernel", "hm_accept_kernel"):
        assert "(%s<T, true>)" % k in src and "(%s<T, false>)" % k in src
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10
    for name in ac.ENTRY_POINTS:
        assert hasattr(lib, name)
    assert hasattr(engine.Engine, "mh_adapt_set") and hasattr(engine.Engine, "mh_adapt_read")
