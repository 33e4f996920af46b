"""gp_mh(chains=M, update='langevin') on the device: cesx_gp_predict_grad against the fp64 numpy restatement at the bar of
cesx_gp_predict, its mean and variance against cesx_gp_predict's bits, the chains against the vectorised numpy restatement,
the exact Gaussian posterior they must leave invariant, device noise, resume, summaries and marginals, and the ABI's states.
What the CPU shows about these bounds (the restatement against itself, the sampler without its correction): NOTEBOOK.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402
import chain_summary_cases as cs  # noqa: E402
from gp_cases import random_gps  # noqa: E402
from gp_langevin_cases import gaussian_bounds_ok, gaussian_problem, np_chains_langevin, np_predict_grad  # noqa: E402

pytestmark = pytest.mark.gpu
FAMILIES = ["RBF", "Matern32", "Matern52"]
LDS_ROWS = 608          # the tile stays in LDS up to 2 J_p + 3 p = 608 (kernels_gpgrad.hip)


def device_grad(enka, X, nugget=True, var=True, dtype="float64"):
    """(mean, var, dmean, dvar, the X the engine holds, gp_predict's mean and var at the same X); gradients (n, M, p)."""
    from ces_amd import emulate as em
    from ces_amd import engine
    img = em.device_image(enka, enka.gpmodels)
    eng = engine.Engine(X.shape[1], img["n"], X.shape[0], dtype=dtype)
    eng.gp_set(img)
    Xd = eng.to_device(np.ascontiguousarray(X.T), X.shape[1], "gp_X")
    m, v, dm, dv = eng.gp_predict_grad(Xd, nugget=nugget, var=var)
    m0, v0 = eng.gp_predict(Xd, nugget=nugget, var=var)
    host = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
    tr = lambda t: None if t is None else t.cpu().numpy().transpose(0, 2, 1)      # noqa: E731
    Xh = eng.to_host(Xd).T.astype(np.float64)
    return host(m), host(v), tr(dm), tr(dv), Xh, host(m0), host(v0)


def check_grad(enka, X, nugget, dtype="float64"):
    m, v, dm, dv, Xh, m0, v0 = device_grad(enka, X, nugget, dtype=dtype)
    _, _, dmr, dvr, sm, sv = np_predict_grad(enka, enka.gpmodels, Xh, nugget)
    assert np.all(np.abs(dm - dmr) <= 1e-9 * (sm + 1e-300)), np.max(np.abs(dm - dmr) / (sm + 1e-300))
    assert np.all(np.abs(dv - dvr) <= 1e-9 * (sv + 1e-300)), np.max(np.abs(dv - dvr) / (sv + 1e-300))
    assert np.array_equal(m, m0) and np.array_equal(v, v0)            # the prediction's bits
    mo, vo, dmo, dvo, _, _, _ = device_grad(enka, X, nugget, var=False, dtype=dtype)
    assert vo is None and dvo is None
    assert np.array_equal(mo, m) and np.array_equal(dmo, dm)          # the mean-only mode


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("scaled", [False, True])
def test_gradients_against_numpy(family, scaled):
    rng = np.random.default_rng(sum(map(ord, family)) + scaled)
    p, n, Jt, M = 3, 5, 77, 203
    enka = random_gps(rng, p, n, Jt, family, scaled)
    X = np.vstack([enka.Ustar.T, rng.standard_normal((M - Jt, p))])     # the first Jt queries on the training inputs
    for nugget in (True, False):
        check_grad(enka, X, nugget)


@pytest.mark.parametrize("Jt,p,M", [(1, 1, 5), (16, 1, 33), (700, 2, 70),
                                    ((LDS_ROWS - 3 * 2) // 32 * 16, 2, 40), ((LDS_ROWS - 3 * 2) // 32 * 16 + 1, 2, 40)])
def test_gradient_shapes(Jt, p, M):
    """Ragged tiles, one block row, the global-workspace path, and the last J_t in LDS (288 at p = 2) and the first beyond."""
    rng = np.random.default_rng(Jt)
    enka = random_gps(rng, p, 2, Jt, "Matern52", mean="Constant")
    X = np.vstack([enka.Ustar.T[:min(Jt, M)], rng.standard_normal((max(0, M - Jt), p))])[:M]
    check_grad(enka, X, True, dtype="float32")


def _mcmc(a, dtype="float64", noise="numpy", seed=1234, stride=1):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    mc.engine_dtype, mc.noise, mc.seed, mc.trace_stride = dtype, noise, seed, stride
    return mc


DELTA = 0.1                 # accept rates 0.50 .. 0.95 over the four likelihoods at 1 024 chains (NOTEBOOK.md)
GAUSS_DELTA = 1.5       # accept rate near 0.6 on gaussian_problem (NOTEBOOK.md)


@pytest.mark.parametrize("mode", ["gamma", "gamma_dense", "var", "gamma_var"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_1024_chains_against_numpy(mode, dtype):
    """The caps of test_gpu_gp.py::test_1024_chains_against_numpy."""
    man, a = load_gold()
    enka = gold_problem(a)
    prior = gold_prior(a)
    Gamma = dict(gamma=a["prob_Gamma_diag"], gamma_dense=a["prob_Gamma_dense"], var=None, gamma_var=a["prob_Gamma_diag"])[mode]
    kw = dict(Gamma=Gamma) if Gamma is not None else {}
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    M, steps = 1024, 20
    mc = _mcmc(a, dtype, stride=steps)
    np.random.seed(5)
    mc.gp_mh(enka, steps, prior, delta=DELTA, chains=M, update="langevin", **kw)
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    scales = DELTA * np.linalg.cholesky(np.cov(enka.Ustar))
    Ur, rate = np_chains_langevin(enka, enka.gpmodels, a["prob_y"], prior, scales, U0, steps, mode.split("_dense")[0],
                                  Gamma if Gamma is not None else np.eye(4), True, 5)
    Ud = mc.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    print("agree %.5f accept device %.6f numpy %.6f" % (agree.mean(), mc.accept, rate.mean()))
    assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(mc.accept - rate.mean()) <= (1e-12 if dtype == "float64" else 0.01)
    assert 0.05 < mc.accept < 0.999                        # (a step that always or never moves compares nothing)


def test_exact_gaussian_posterior_is_invariant():
    """16 384 chains from exact posterior draws, 30 Langevin steps, accept rate near 0.6: the pooled mean and covariance stay
    within 5 standard errors.  (The same sampler with its correction dropped fails this on the CPU: NOTEBOOK.md.)"""
    from ces_amd import sample
    M = 16384
    enka, prior, y, Gamma, mp, Cp = gaussian_problem(M)
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = y
    mc.noise = "device"
    mc.trace_stride = 30
    mc.gp_mh(enka, 30, prior, delta=GAUSS_DELTA, chains=M, start="ensemble", update="langevin", Gamma=Gamma)
    ok, zm, zc = gaussian_bounds_ok(mc.samples[:, -1, :], mp, Cp)
    print("accept %.4f worst mean z %.3f worst cov z %.3f" % (mc.accept, zm, zc))
    assert 0.5 < mc.accept < 0.7, mc.accept
    assert ok, (zm, zc)


def test_device_noise_bit_identical_and_exact_resume():
    man, a = load_gold()

    def run(splits):
        enka = gold_problem(a)
        mc = _mcmc(a, noise="device", seed=99)
        for s in splits:
            mc.gp_mh(enka, s, gold_prior(a), delta=DELTA, chains=257, update="langevin")
        return mc.samples
    one = run([12])
    assert np.array_equal(one, run([12]))
    two = run([5, 7])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
    assert not np.array_equal(one[:, 0, :], one[:, -1, :])


def test_summary_and_marginals_equal_numpy_on_the_trace():
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    M, steps = 64, 24
    kw = dict(delta=DELTA, chains=M, update="langevin", Gamma=a["prob_Gamma_diag"])
    tr = _mcmc(a, noise="device", seed=7)
    tr.gp_mh(enka, steps, gold_prior(a), **kw)
    sm = _mcmc(a, noise="device", seed=7)
    sm.gp_mh(enka, steps, gold_prior(a), summary=True, marginals=True, **kw)
    assert np.array_equal(sm.samples[:, -1, :], tr.samples[:, -1, :]) and tr.accept == sm.accept
    draws = cs.draws_of(tr.samples, steps, 1, 0)            # (N, p, M): every state but the start
    assert draws.shape == (steps, 2, M)
    ref = cs.ref_raw(draws)
    want, bounds = cs.finalise_ref(ref), cs.summary_bounds(ref)
    assert sm.summary["n"] == steps and sm.summary["chains"] == M
    for k, b in bounds.items():
        assert np.all(np.abs(sm.summary[k] - want[k]) <= b), (k, float(np.max(np.abs(sm.summary[k] - want[k]) / b)))
    mg = sm.marginals
    assert mg["n"] == steps and mg["chains"] == M and mg["hist1d"].sum() > 0
    for r in range(2):
        x = draws[:, r, :].ravel()
        assert np.array_equal(mg["hist1d"][r], np.histogram(x, bins=mg["edges"][r])[0])
        assert mg["below"][r] == (x < mg["edges"][r, 0]).sum() and mg["above"][r] == (x > mg["edges"][r, -1]).sum()


def test_abi_states_leave_the_chains_untouched():
    """Every ESTATE / EINVAL / EUNSUPPORTED case of cesx_gp_langevin_* and cesx_gp_predict_grad returns its code, launches
    nothing and leaves U and cesx_mh_phi as they were."""
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    man, a = load_gold()
    enka = gold_problem(a)
    p, n, M = 2, 4, 30
    img = em.device_image(enka, enka.gpmodels)
    eng = engine.Engine(p, n, M, dtype="float64")
    lib, h = eng.lib, eng._h
    U = eng.to_device(np.ascontiguousarray(enka.Ustar[:, :M]), p, "U").clone()
    P = eng.empty(p)
    new = lambda *s: torch.zeros(s, dtype=torch.float64, device=eng.device)      # noqa: E731
    mean, var, dm, dv = new(n, M), new(n, M), new(n, p, M), new(n, p, M)
    ptr = lambda t: t.data_ptr()      # noqa: E731
    start = lambda mode=0: lib.cesx_gp_langevin_start(h, mode, ptr(U), ptr(mean), ptr(var), ptr(dm), ptr(dv), None)      # noqa: E731
    propose = lambda: lib.cesx_gp_langevin_propose(h, 0, ptr(U), None, ptr(P), None)      # noqa: E731
    accept = lambda mode=0: lib.cesx_gp_langevin_accept(h, mode, 0, ptr(U), ptr(P), ptr(mean), ptr(var), ptr(dm), ptr(dv), None, None)      # noqa: E731
    grad = lambda: lib.cesx_gp_predict_grad(h, ptr(U), ptr(mean), ptr(var), ptr(dm), ptr(dv), 1, None)      # noqa: E731
    S = np.ascontiguousarray(0.1 * np.eye(p))
    mu, Sig = np.asarray(a["prob_mu"], dtype=np.float64), np.asarray(a["prob_Sigma"], dtype=np.float64)

    # nothing installed: no problem, no proposal, no emulator
    assert grad() == engine.ESTATE
    assert start() == engine.ESTATE and propose() == engine.ESTATE and accept() == engine.ESTATE
    eng.set_problem(np.asarray(a["prob_y"], dtype=np.float64), a["prob_Gamma_diag"], mu, Sig, mu)
    assert start() == engine.ESTATE                        # no proposal
    eng.mh_set_proposal(None, S)
    eng.gp_set(img)
    assert start() == engine.ESTATE                        # a random-walk proposal is no Langevin proposal
    eng.mh_set_proposal("langevin", S)
    assert propose() == engine.ESTATE and accept() == engine.ESTATE      # no start
    # a Matern12 emulator has no gradient
    img12 = em.device_image(enka, gold_problem(a, family="Matern12").gpmodels)
    eng.gp_set(img12)
    assert grad() == engine.EUNSUPPORTED
    eng.gp_set(img)

    # a started run, then every refusal against its state
    eng.gp_predict_grad(U, out=(mean, var, dm, dv))
    eng.gp_langevin_start("gamma", U, mean, var, dm, dv)
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert accept() == engine.ESTATE                       # no propose since the start
    for mode in (engine.GP_MODES["dense"], engine.GP_MODES["proj"], 17):
        assert start(mode) == engine.EINVAL
    assert propose() == engine.OK
    for mode in (engine.GP_MODES["dense"], engine.GP_MODES["proj"], 17):
        assert accept(mode) == engine.EINVAL
    assert lib.cesx_gp_run(h, 0, 0, 1, 1, 1, ptr(U), None, None, None, None) == engine.EINVAL
    assert lib.cesx_gp_start(h, 0, ptr(U), ptr(mean), ptr(var), None) == engine.EINVAL
    assert lib.cesx_mh_propose(h, 0, ptr(U), None, ptr(P), None) == engine.EINVAL
    assert lib.cesx_gp_langevin_propose(h, 1 << 31, ptr(U), None, ptr(P), None) == engine.EINVAL
    assert lib.cesx_gp_langevin_propose(h, 0, ptr(U), None, ptr(U), None) == engine.EINVAL
    assert lib.cesx_gp_predict_grad(h, ptr(U), ptr(mean), None, ptr(dm), ptr(dv), 1, None) == engine.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0)
    steps, rate = eng.mh_stats()
    assert steps == 0 and rate == 0.0
    # and the run goes on: the proposal's rows, then the accept step
    eng.gp_predict_grad(P, out=(mean, var, dm, dv))
    assert accept() == engine.OK
    assert eng.mh_stats()[0] == 1
    # a dense Gamma has no variance mode
    eng.set_problem(np.asarray(a["prob_y"], dtype=np.float64), a["prob_Gamma_dense"], mu, Sig, mu)
    eng.mh_set_proposal("langevin", S)
    assert start(engine.GP_MODES["var"]) == engine.EINVAL
    eng.close()
