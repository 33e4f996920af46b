"""The Darcy forward map on the device (cesx_darcy_*, ces_amd/csrc/kernels_darcy.hip) against the host map.

The yardstick everywhere is the host map ``ces_amd.darcy.model.__call__`` in fp64, particle by particle (for an fp32 engine
evaluated at the fp32-rounded inputs); the device path is never compared with itself.  Parity is per particle,

    max|g_dev - g_host| <= 16 cond_2(A) 2^-52 max|g_host|      (+ 2^-23 max|g_host| for the output rounding of an fp32 engine),

cond_2(A) from ``darcy.assemble_gwf`` on the host: 16 is ~25x the 0.65 measured between two CPU LU solvers on the same
draws (scipy's ``solve_banded`` against ``spsolve``); the device's pivot sequence may break ties differently.  The largest
observed ratio error / (cond eps max|g|) of a run is printed when the module's tests are over (NOTEBOOK.md records it).
"""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err  # noqa: E402
import darcy_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {"ratio": 0.0, "case": None}
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield engine
    print("\n[darcy] worst |g_dev - g_host| / (cond_2(A) 2^-52 max|g_host|) over the fp64 cases of this run: %.3g at %s"
          % (WORST["ratio"], WORST["case"]))


def _check(G, ref, dtype, J, case):
    """Every particle of G (n_obs, J) within its bound of the host reference; records the worst fp64 ratio."""
    tol, gmax, cond = dc.tolerance(ref, dtype, J)
    err = np.max(np.abs(G - ref["G"][:, :J]), axis=0)
    if np.dtype(dtype) == np.float64:
        ratio = float(np.max(err / (cond * EPS * gmax)))
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, case=case)
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, (case, "particles", bad[:5], "err", err[bad[:5]], "bound", tol[bad[:5]], "cond", cond[bad[:5]])


@pytest.mark.parametrize("J", [1, 65, 130])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scale", dc.SCALES)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "K%d-p%d-n%d" % s)
def test_map_against_the_host(eng_mod, shape, scale, dtype, J):
    K, p, n_obs = shape
    ref = dc.reference(K, p, n_obs, scale, dtype)
    eng = eng_mod.Engine(p, n_obs, J, dtype=dtype)
    mdl = dc.make_model(K, p, n_obs)
    U = eng.to_device(np.array(ref["U"][:, :J]), p, "U")
    G = mdl.forward_device(eng, U).cpu().numpy().astype(np.float64)
    assert G.shape == (n_obs, J) and np.all(np.isfinite(G))
    _check(G, ref, dtype, J, (shape, scale, dtype, J))
    eng.close()


def _host(mdl, U):
    parts = [dc.host_parts(mdl, U[:, j]) for j in range(U.shape[1])]
    return dict(G=np.stack([q[0] for q in parts], axis=1), cond=np.array([q[1] for q in parts]))


def test_reinstall(eng_mod):
    """One engine, the map changed between calls: obs_index, tau, alpha and the rank order each re-install and give the new
    host values; a p that no longer matches the engine's is a ValueError that leaves nothing stale (an engine's p is
    fixed: that is all a change of p can mean on one engine); two models alternate; invalidate_device() re-installs."""
    from ces_amd import darcy
    K, p, n_obs, J = 8, 10, 12, 5
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    rng = np.random.default_rng(8)
    Uh = 3.0 * rng.standard_normal((p, J))
    U = eng.to_device(Uh, p, "U")
    mdl = dc.make_model(K, p, n_obs)

    def check(m, case):
        G = m.forward_device(eng, U).cpu().numpy()
        _check(G, _host(m, Uh), "float64", J, case)
        return G
    g0 = check(mdl, "reinstall: first")
    mdl.obs_index = np.roll(mdl.obs_index, 5)
    g1 = check(mdl, "reinstall: obs_index")
    assert not np.array_equal(g0, g1)
    mdl.tau = 4.5
    mdl.set_rank()
    g2 = check(mdl, "reinstall: tau")
    assert not np.array_equal(g1, g2)
    mdl.alpha = 2.5
    mdl.set_rank()
    check(mdl, "reinstall: alpha")
    mdl.rank = np.concatenate([mdl.rank[:p][::-1], mdl.rank[p:]])
    check(mdl, "reinstall: rank")
    mdl.p = p + 2
    with pytest.raises(ValueError, match="p = 12 differs"):
        mdl.forward_device(eng, U)
    mdl.p = p
    check(mdl, "reinstall: p restored")
    other = darcy.model_trunc(Nmesh=float(K), p=p, tau=2.0)
    other.obs_index = np.arange(n_obs)[::-1].copy()
    for k in range(2):
        check(other, "reinstall: other model %d" % k)
        check(mdl, "reinstall: first model %d" % k)
    token = eng._darcy_token
    mdl.forward_device(eng, U)
    assert eng._darcy_token is token                     # nothing changed: not installed again
    mdl.invalidate_device()
    check(mdl, "reinstall: invalidated")
    assert eng._darcy_token is not token
    eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_out_and_bit_reproducibility(eng_mod, dtype):
    K, p, n_obs, J = 16, 64, 50, 130
    ref = dc.reference(K, p, n_obs, 10, dtype)
    eng = eng_mod.Engine(p, n_obs, J, dtype=dtype)
    mdl = dc.make_model(K, p, n_obs)
    U = eng.to_device(np.array(ref["U"]), p, "U")
    G = eng.empty(n_obs)
    G.fill_(7.0)
    ret = mdl.forward_device(eng, U, out=G)
    assert ret is G
    a = G.cpu().numpy().copy()
    _check(a.astype(np.float64), ref, dtype, J, ("out=", dtype))
    b = mdl.forward_device(eng, U).cpu().numpy()
    c = mdl.forward_device(eng, U, out=G).cpu().numpy()
    assert a.tobytes() == b.tobytes() == c.tobytes()
    eng.close()


class _ZeroBlockModel:
    """Mixin: the descriptor with S replaced by a small-integer matrix whose rows sum to zero.  For xi = 0, exp(theta) is the
    all-ones matrix EXACTLY (exp(0) = 1), S exp(theta) S^T is a sum of +-1 that cancels EXACTLY in any order, and A -- the
    whole matrix, its leading diagonal block included -- is exactly zero: the first pivot is an exact zero on the host and
    on the device alike."""
    S_EXACT = np.array([[1.0, -1, 0, 0], [0, 1, -1, 0], [0, 0, 1, -1], [1, 0, 0, -1]])

    def device_descriptor(self, n_obs=None):
        d = super().device_descriptor(n_obs)
        d["S"] = self.S_EXACT.copy()
        return d


def test_singular_particle(eng_mod):
    """K = 4, m = 2: one column is crafted so that the first pivot is exactly zero (see _ZeroBlockModel).  The CPU confirms
    the construction -- A == 0 exactly, scipy's banded LU reports the singular matrix, its dense LU the zero diagonal --; on
    the device LinAlgError names the particle, that particle's outputs are NaN and the other columns are still right
    (against the same descriptor applied in numpy with scipy's banded LU, the host yardstick of a map that is no longer
    ``model.__call__``).  An arithmetic status path: nothing faults."""
    import warnings
    import torch
    from scipy.linalg import LinAlgWarning, lu_factor
    from ces_amd import darcy

    class M(_ZeroBlockModel, darcy.model):
        pass
    K, p, n_obs, J, bad = 4, 16, 5, 6, 2
    mdl = M(Nmesh=float(K))
    mdl.obs_index = np.array([5, 15, 0, 9, 10])
    desc = mdl.device_descriptor(n_obs)
    rng = np.random.default_rng(5)
    Uh = rng.standard_normal((p, J))
    Uh[:, bad] = 0.0
    # the CPU's view of the crafted column
    a = desc["S"] @ np.exp(desc["D"] @ (desc["coef"] * Uh[:, bad].reshape(K, K)) @ desc["D"].T) @ desc["S"].T
    A = darcy.assemble_gwf(a).toarray()
    assert np.all(a == 0.0) and np.all(A == 0.0)
    with pytest.raises(np.linalg.LinAlgError):
        dc.apply_descriptor(desc, Uh[:, bad])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        lu, _ = lu_factor(A)
    assert lu[0, 0] == 0.0 and any(issubclass(x.category, LinAlgWarning) for x in w)

    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    U = eng.to_device(Uh, p, "U")
    G = eng.empty(n_obs)
    with pytest.raises(np.linalg.LinAlgError, match="particle %d " % bad):
        mdl.forward_device(eng, U, out=G)
    torch.cuda.synchronize()
    Gh = G.cpu().numpy()
    assert np.all(np.isnan(Gh[:, bad]))
    good = [j for j in range(J) if j != bad]
    want = np.stack([dc.apply_descriptor(desc, Uh[:, j]) for j in good], axis=1)
    cond = []
    for j in good:
        aj = desc["S"] @ np.exp(desc["D"] @ _kl(desc, Uh[:, j]) @ desc["D"].T) @ desc["S"].T
        cond.append(np.linalg.cond(darcy.assemble_gwf(aj).toarray()))
    _check(Gh[:, good], dict(G=want, cond=np.array(cond)), "float64", len(good), "singular: the other columns")
    # without the crafted column nothing is reported
    Uh2 = Uh.copy()
    Uh2[:, bad] = Uh[:, 0]
    G2 = mdl.forward_device(eng, eng.to_device(Uh2, p, "U2")).cpu().numpy()
    assert np.all(np.isfinite(G2)) and np.array_equal(G2[:, bad], G2[:, 0])
    eng.close()


def _kl(desc, xi):
    K = desc["K"]
    Xi = np.zeros(K * K)
    Xi[desc["scatter"]] = xi
    L = desc["coef"] * Xi.reshape(K, K)
    L[0, 0] = 0.0
    return L


def _run_problem():
    K, p, n_obs, J = 8, 10, 12, 70
    mdl = dc.make_model(K, p, n_obs)
    mdl.set_initial()
    rng = np.random.default_rng(12)
    gamma = 0.005
    Gamma = gamma ** 2 * np.identity(n_obs)
    y = mdl(mdl.ustar) + gamma * rng.standard_normal(n_obs)
    return mdl, rng, Gamma, y, (K, p, n_obs, J)


@pytest.mark.parametrize("update", ["aldi", "eks"])
def test_device_resident_run(eng_mod, update):
    """``sampling.run`` with the Darcy ensemble resident on the device (the device map, ``xis=`` given) against the same
    run with ``device_loop = False`` (the host map through G_ens, the same ``xis``): Uall and Gall to 1e-9 relative (the fp64
    map agrees to ~1e-13 and the update to ~1e-12, both amplified over three steps), metrics['t'] to 1e-8."""
    from ces_amd.calibrate import sampling
    mdl, rng, Gamma, y, (K, p, n_obs, J) = _run_problem()
    T = 3
    U0 = rng.standard_normal((p, J))
    xis = rng.standard_normal((T, p, J))
    runs = []
    for device_loop in (True, False):
        eks = sampling(p=p, n_obs=n_obs, J=J)
        eks.T, eks.ustar, eks.mu, eks.sigma = T, mdl.ustar.reshape(p, 1), np.zeros((p, 1)), 100.0 * np.identity(p)
        eks.device_loop = device_loop
        assert eks._device_loop_ok(mdl, False, dict(xis=xis, update=update)) == device_loop
        eks.run(y, np.copy(U0), mdl, Gamma, np.linalg.cholesky(Gamma), update=update, t_tol=1e9, xis=xis)
        runs.append(eks)
    dev, host = runs
    assert dev.Uall.shape == host.Uall.shape == (T + 1, p, J) and dev.Gall.shape == host.Gall.shape == (T + 1, n_obs, J)
    eu, eg = rel_err(dev.Uall, host.Uall), rel_err(dev.Gall, host.Gall)
    print("\n[darcy] device-resident run, %s: rel err Uall %.3g Gall %.3g" % (update, eu, eg))
    assert eu < 1e-9 and eg < 1e-9
    assert len(dev.metrics["t"]) == T and np.allclose(dev.metrics["t"], host.metrics["t"], rtol=1e-8, atol=0.0)


def _sampler(mdl, Gamma, y, p, n_obs, M):
    from ces_amd import calibrate, sample
    rng = np.random.default_rng(4)
    enka = calibrate.enka(p, n_obs, 130)
    enka.Ustar = mdl.ustar.reshape(p, 1) + 0.3 * rng.standard_normal((p, 130))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, y
    prior = stats.multivariate_normal(mean=np.zeros(p), cov=100.0 * np.identity(p))
    return mc, enka, prior


def test_sampler_one_chain_equals_the_host_chain(eng_mod):
    """MCMC.model_mh(chains=1, noise='numpy') under a fixed np.random.seed against the host model_mh (no chains=) under the same
    seed: the same draws in the same order, samples to 1e-10, accept identical."""
    mdl, _, Gamma, y, (K, p, n_obs, J) = _run_problem()
    out = []
    for chains in (1, None):
        mc, enka, prior = _sampler(mdl, Gamma, y, p, n_obs, 1)
        np.random.seed(31)
        kw = {} if chains is None else dict(chains=chains)
        mc.model_mh(mdl, 30, prior, enka, Gamma, delta=1.0, **kw)
        out.append(mc)
    dev, host = out
    assert dev.samples.shape == host.samples.shape == (p, 31)
    err = rel_err(dev.samples, host.samples)
    print("\n[darcy] model_mh chains=1 against the host chain: rel err %.3g, accept %.3f" % (err, host.accept))
    assert err < 1e-10 and dev.accept == host.accept
    assert 0.0 < host.accept < 1.0                         # (both branches of the test were taken: 22 of 30 on the host)


def test_sampler_many_chains_on_device_noise(eng_mod):
    mdl, _, Gamma, y, (K, p, n_obs, J) = _run_problem()
    out = []
    for _ in range(2):
        mc, enka, prior = _sampler(mdl, Gamma, y, p, n_obs, 130)
        mc.noise = "device"
        mc.model_mh(mdl, 30, prior, enka, Gamma, delta=1.0, chains=130, start="ensemble")
        out.append(mc)
    a, b = out
    assert a.samples.shape == (p, 31, 130) and np.all(np.isfinite(a.samples))
    assert a.samples.tobytes() == b.samples.tobytes() and a.accept == b.accept
    assert np.any(a.samples[:, -1, :] != a.samples[:, 0, :])


def test_overflowing_particle_is_not_called_singular(eng_mod):
    """exp(theta) overflows for one column: the host map has no finite value there (its spline refuses the non-finite field), the device reports the particle as
    NOT FINITE (not as a zero pivot), writes NaN for it and leaves the other columns right."""
    import warnings
    import torch
    K, p, n_obs, J, bad = 8, 10, 12, 5, 3
    mdl = dc.make_model(K, p, n_obs)
    rng = np.random.default_rng(2)
    Uh = rng.standard_normal((p, J))
    Uh[:, bad] = 1e5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            try:
                g_host = mdl(Uh[:, bad])
            except Exception:                                # (scipy may refuse the non-finite matrix outright)
                g_host = np.full(n_obs, np.nan)
    assert not np.any(np.isfinite(g_host))
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    G = eng.empty(n_obs)
    with pytest.raises(np.linalg.LinAlgError, match="particle %d is not finite" % bad):
        mdl.forward_device(eng, eng.to_device(Uh, p, "U"), out=G)
    torch.cuda.synchronize()
    Gh = G.cpu().numpy()
    assert np.all(np.isnan(Gh[:, bad]))
    good = [j for j in range(J) if j != bad]
    _check(Gh[:, good], _host(mdl, Uh[:, good]), "float64", len(good), "overflow: the other columns")
    eng.close()
