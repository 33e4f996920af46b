"""The device path of MCMC.model_mh (chains=M; cesx_mh_* and mh_accept_kernel) on the MI355X: the reference's chains
(tests/golden/mcmc.npz), many chains against a vectorised numpy restatement, stationarity and convergence against the
analytic Gaussian posterior of a linear map, and reproducibility."""
import numpy as np
import pytest
from scipy import stats

from test_mcmc_host import load_cases, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import build, engine
    build.build_lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def moves(samples):
    """Which steps of a (p, n) chain changed the state (= the accept sequence)."""
    return np.any(np.diff(samples, axis=1) != 0, axis=0)


@pytest.mark.parametrize("case", [c["name"] for c, _ in load_cases()])
def test_one_device_chain_reproduces_the_reference(eng_mod, case):
    c, a = next((c, a) for c, a in load_cases() if c["name"] == case)
    mc = run_case(c, a, chains=1, start="mean")
    ref = a["samples"]
    assert mc.samples.shape == ref.shape
    assert np.array_equal(moves(mc.samples), moves(ref))
    np.testing.assert_allclose(mc.samples, ref, rtol=1e-9, atol=1e-12)
    assert mc.accept == pytest.approx(float(a["accept"]), abs=1e-15)
    assert mc.accept_chains.shape == (1,)


def _problem(rng, p, n, dense_sigma):
    A = rng.standard_normal((n, p)) / np.sqrt(p)
    gam = 0.1 + 0.1 * rng.random(n)
    y = A @ (0.5 * rng.standard_normal(p)) + np.sqrt(gam) * rng.standard_normal(n)
    mu = 0.1 * rng.standard_normal(p)
    if dense_sigma:
        B = rng.standard_normal((p, p)) / np.sqrt(p)
        Sigma = 0.5 * (B @ B.T) + 0.5 * np.eye(p)
    else:
        Sigma = np.diag(0.5 + rng.random(p))
    return A, y, np.diag(gam), mu, Sigma


@pytest.mark.parametrize("p", [64, 256])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_many_chains_against_numpy(eng_mod, p, dtype):
    """M = 1024 chains, injected xi and log u for 20 steps, against the reference's arithmetic on all chains at once."""
    import torch
    rng = np.random.default_rng(p + (1 if dtype == "float32" else 0))
    n, M, steps = p, 1024, 20
    A, y, Gamma, mu, Sigma = _problem(rng, p, n, dense_sigma=(p == 64))
    S = np.sqrt(2 * 0.15 / n) * np.linalg.cholesky(Sigma)
    eng = eng_mod.Engine(p, n, M, dtype=dtype)
    eng.set_problem(y, Gamma, mu, Sigma, mu)
    eng.forward_set_lineal(A)
    eng.mh_set_proposal(None, S)
    Sinv, gw = np.linalg.inv(Sigma), 1.0 / np.diag(Gamma)

    def phi(X):
        r = A @ X - y[:, None]
        d = X - mu[:, None]
        return 0.5 * (gw[:, None] * r * r).sum(0) + 0.5 * np.einsum("ij,ij->j", d, Sinv @ d)

    U0 = mu[:, None] + 0.3 * rng.standard_normal((p, M))
    U = eng.to_device(U0, p).clone()
    G, P, GP = eng.empty(n), eng.empty(p), eng.empty(n)
    eng.forward_apply(U, out=G)
    eng.mh_start(U, G)
    Uref = np.array(U.cpu().numpy(), dtype=np.float64)
    phi_ref = phi(Uref)
    tied = np.zeros(M, dtype=bool)
    for k in range(steps):
        xi = rng.standard_normal((p, M))
        logu = np.log(rng.random(M))
        eng.mh_propose(k, U, xi=eng.to_device(xi, p), out=P)
        Pref = Uref + S @ xi
        eng.forward_apply(P, out=GP)
        eng.mh_accept(k, U, P, GP, logu=torch.as_tensor(logu, dtype=torch.float64, device=eng.device))
        phi_p = phi(Pref)
        margin = phi_ref - phi_p - logu
        acc = logu < phi_ref - phi_p
        Uref[:, acc] = Pref[:, acc]
        phi_ref[acc] = phi_p[acc]
        got = U.cpu().numpy().astype(np.float64)
        if dtype == "float64":
            np.testing.assert_allclose(got, Uref, rtol=1e-9, atol=1e-9)
        else:
            tied |= np.abs(margin) <= 1e-3 * np.maximum(1.0, np.abs(phi_ref))
            ok = ~tied
            np.testing.assert_allclose(got[:, ok], Uref[:, ok], rtol=1e-3, atol=1e-3)
    nsteps, rate, per = eng.mh_stats(per_chain=True)
    assert nsteps == steps and 0.02 < rate < 0.98, rate
    assert int(per.sum()) == round(rate * steps * M)
    if dtype == "float32":
        # (|phi| is O(100) here, so the band |margin| <= 1e-3 |phi| is wide and 20 steps put many chains in it once)
        assert (~tied).sum() >= 128


def _posterior(A, y, Gamma, mu, Sigma):
    Gi, Si = np.linalg.inv(Gamma), np.linalg.inv(Sigma)
    Cp = np.linalg.inv(A.T @ Gi @ A + Si)
    Cp = 0.5 * (Cp + Cp.T)
    return Cp @ (A.T @ Gi @ y + Si @ mu), Cp


def test_stationarity_at_the_benchmark_shape(eng_mod):
    """p = n = 256, fp32, dense Sigma, 65 536 chains started from exact posterior draws, 50 RW steps of device noise."""
    from ces_amd import calibrate, sample, utils
    rng = np.random.default_rng(11)
    p = n = 256
    M, steps = 65536, 50
    A, y, Gamma, mu, Sigma = _problem(rng, p, n, dense_sigma=True)
    m, Cp = _posterior(A, y, Gamma, mu, Sigma)
    U0 = m[:, None] + np.linalg.cholesky(Cp) @ rng.standard_normal((p, M))
    enka = calibrate.enka(p, n, M)
    enka.Ustar = U0
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, y
    mc.engine_dtype, mc.noise, mc.trace_stride = "float32", "device", steps
    mc.model_mh(utils.lineal(A), steps, stats.multivariate_normal(mean=mu, cov=Sigma), enka, Gamma,
                delta=2.38 / np.sqrt(p), chains=M, start="ensemble")
    assert mc.samples.shape == (p, 2, M)
    X = mc.samples[:, -1, :]
    assert 0.1 < mc.accept < 0.6, mc.accept
    assert np.any(X != mc.samples[:, 0, :])
    se = np.sqrt(np.diag(Cp) / M)
    z = np.abs(X.mean(1) - m) / se
    assert z.max() < 6.0, z.max()
    rel = np.abs(X.var(1, ddof=1) / np.diag(Cp) - 1.0)
    assert rel.max() < 0.05, rel.max()
    eng = mc._mh_eng
    nsteps, rate, per = eng.mh_stats(per_chain=True)
    assert nsteps == steps and int(per.sum()) == round(mc.accept * steps * M)
    np.testing.assert_allclose(mc.accept_chains * steps, per)


def test_convergence_of_the_small_problem(eng_mod):
    """The fixtures' p = 2 problem: 65 536 chains from the prior, 500 steps, against the analytic posterior."""
    from ces_amd import calibrate, sample, utils
    c, a = next((c, a) for c, a in load_cases() if c["name"] == "rw_diag")
    rng = np.random.default_rng(5)
    M, steps = 65536, 500
    m, Cp = _posterior(a["A"], a["y"], a["Gamma"], a["mu"], a["Sigma"])
    enka = calibrate.enka(2, c["n_obs"], M)
    enka.Ustar = a["mu"][:, None] + np.linalg.cholesky(a["Sigma"]) @ rng.standard_normal((2, M))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["y"]
    mc.noise, mc.trace_stride = "device", steps
    mc.model_mh(utils.lineal(a["A"]), steps, stats.multivariate_normal(mean=a["mu"], cov=a["Sigma"]), enka, a["Gamma"],
                delta=1.7 * np.sqrt(np.diag(Cp).mean()), enka_scaling=False, chains=M, start="ensemble")
    X = mc.samples[:, -1, :]
    se = np.sqrt(np.diag(Cp) / M)
    assert np.all(np.abs(X.mean(1) - m) < 6 * se), (X.mean(1), m, se)
    C = np.cov(X)
    assert np.all(np.abs(C - Cp) < 0.04 * np.sqrt(np.outer(np.diag(Cp), np.diag(Cp)))), (C, Cp)


def _chain(seed, steps, resume_at=None):
    from ces_amd import calibrate, sample, utils
    rng = np.random.default_rng(21)
    p = n = 64
    M = 4096
    A, y, Gamma, mu, Sigma = _problem(rng, p, n, dense_sigma=True)
    enka = calibrate.enka(p, n, M)
    enka.Ustar = mu[:, None] + 0.3 * rng.standard_normal((p, M))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, y
    mc.engine_dtype, mc.noise, mc.seed, mc.trace_stride = "float32", "device", seed, 10
    args = (utils.lineal(A), None, stats.multivariate_normal(mean=mu, cov=Sigma), enka, Gamma)
    kw = dict(delta=0.5, chains=M, start="ensemble")
    if resume_at is None:
        mc.model_mh(args[0], steps, *args[2:], **kw)
    else:
        mc.model_mh(args[0], resume_at, *args[2:], **kw)
        mc.model_mh(args[0], steps - resume_at, *args[2:], **kw)
    return mc


def test_runs_are_reproducible_and_resume_exactly(eng_mod):
    a, b = _chain(7, 100), _chain(7, 100)
    assert np.array_equal(a.samples, b.samples) and a.accept == b.accept
    r = _chain(7, 100, resume_at=50)
    assert r.samples.shape == a.samples.shape
    assert np.array_equal(r.samples, a.samples)
    assert not np.array_equal(_chain(8, 100).samples[:, -1], a.samples[:, -1])


def test_mh_noise_is_its_own_counter_domain(eng_mod):
    import torch
    p, n, M = 64, 64, 4096
    for dtype in ("float32", "float64"):
        eng = eng_mod.Engine(p, n, M, dtype=dtype)
        eng.set_problem(np.zeros(n), np.eye(n), np.zeros(p), np.eye(p), np.zeros(p))
        eng.mh_set_proposal(None, np.eye(p))
        U = torch.zeros((p, M), dtype=eng.torch_dtype, device=eng.device)
        xi_mh = eng.mh_propose(3, U).cpu().numpy().astype(np.float64)          # P = 0 + I xi
        xi_eks = eng.draw_noise(3).cpu().numpy().astype(np.float64)
        assert abs(xi_mh.mean()) < 0.01 and abs(xi_mh.std() - 1.0) < 0.01
        assert np.corrcoef(xi_mh.ravel(), xi_eks.ravel())[0, 1] < 0.01
        assert not np.any(xi_mh == xi_eks)
        assert not np.array_equal(xi_mh, eng.mh_propose(4, U).cpu().numpy().astype(np.float64))
