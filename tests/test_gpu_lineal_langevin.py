"""model_mh(chains=M, update='langevin') for the linear maps on the device (cesx_mh_langevin_lineal_*, kernels_lvlin.hip): g term
by term against fp64 numpy, phi against the random walk's bit for bit, the wide path against the Jacobian path, the chains
against numpy, the invariance of the exact posterior, and the sampler's contracts (reproducibility, resume, shards, summaries,
NaN, ABI states).  Cases, references and bounds: tests/lineal_langevin_cases.py."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_summary_cases as cs  # noqa: E402
import lineal_langevin_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 1e-9                                                 # the caps of test_gpu_map_langevin.py


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def _engine(eng_mod, prob, J, dtype, update="langevin", **kw):
    eng = eng_mod.Engine(prob["p"], prob["n"], J, dtype=dtype, seed=77, **kw)
    eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["Sigma"], prob["mu"])
    eng.mh_set_proposal(update, lc.scales(prob))
    return eng


def _states(prob, J, dtype, seed=9):
    """J states from the ensemble's law, already rounded to the engine dtype: the U the engine holds."""
    return lc.exact_draws(prob, J, seed).astype(np.dtype(dtype)).astype(np.float64)


def _started(eng_mod, prob, J, dtype, U0=None, **kw):
    """An engine with the problem, the Langevin proposal, the model's images and the start states scored: (eng, model, U, G)."""
    eng = _engine(eng_mod, prob, J, dtype, **kw)
    model = lc.model_of(prob)
    model.langevin_device(eng)
    U = eng.to_device(_states(prob, J, dtype) if U0 is None else U0, prob["p"], "U0").clone()
    G = model.forward_device(eng, U).clone()
    eng.mh_langevin_lineal_start(U, G)
    return eng, model, U, G


# ---- 1. g, term by term ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", list(lc.CASES))
def test_g_term_by_term(eng_mod, name, dtype):
    """After _lineal_start, _g() against fp64 numpy at the U the engine holds, elementwise within c u_T mag (lc.g_bound), for
    J in {1, 63, 64, 65, 257} and the four forms of Gamma and Sigma.  Measured worst err / bound: NOTEBOOK.md."""
    worst = 0.0
    for forms in lc.FORMS:
        prob = lc.problem(name, *forms)
        S = lc.scales(prob)
        for J in (1, 63, 64, 65, 257):
            eng, model, U, G = _started(eng_mod, prob, J, dtype)
            Uh = eng.to_host(U).astype(np.float64)
            g = eng.mh_langevin_lineal_g()
            assert g.shape == (prob["p"], J)
            _, want = lc.np_phi_g(prob, S, Uh)
            ratio = np.abs(g - want) / lc.g_bound(prob, S, Uh, dtype)
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1), (name, forms, J, dtype, float(ratio.max()))
            eng.close()
    print("\n[lineal langevin] g %s %s: worst err / bound %.4g" % (name, dtype, worst))


# ---- 2. phi is the random walk's ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["lineal-17x33", "log-5x3"])
def test_phi_is_the_random_walks_bit_for_bit(eng_mod, name, dtype):
    for forms in lc.FORMS:
        prob = lc.problem(name, *forms)
        for J in (65, 257):
            eng, model, U, G = _started(eng_mod, prob, J, dtype)
            phi = eng.mh_phi()
            rw = _engine(eng_mod, prob, J, dtype, update=None)
            Ur, Gr = rw.to_device(eng.to_host(U), prob["p"], "U").clone(), rw.to_device(eng.to_host(G), prob["n"], "G").clone()
            rw.mh_start(Ur, Gr)
            assert np.array_equal(phi, rw.mh_phi()) and np.all(np.isfinite(phi)) and np.all(phi > 0), (name, forms, J)
            eng.close()
            rw.close()


# ---- 3. the wide path equals the Jacobian path ----------------------------------------------------------------------------------

def test_wide_path_equals_the_jacobian_path(eng_mod):
    """p = 5, n = 3, J = 65, fp64, lineal, 7 single steps with device noise, seed 77: the new entry points against
    cesx_mh_langevin_start / _propose / _accept fed G in fp64 and DG[i][q][j] = A[i][q]."""
    import torch
    prob = lc.problem("lineal-5x3", True, True)
    p, n, J, steps = 5, 3, 65, 7
    a, model, Ua, _ = _started(eng_mod, prob, J, "float64")
    b = _engine(eng_mod, prob, J, "float64")
    mb = lc.model_of(prob)
    Ub = b.to_device(a.to_host(Ua), p, "U").clone()
    DG = torch.as_tensor(np.ascontiguousarray(np.repeat(prob["A"][:, :, None], J, axis=2)), device=b.device)
    b.mh_langevin_start(Ub, mb.forward_device(b, Ub), DG)
    Pa, Pb = a.empty(p), b.empty(p)
    for k in range(steps):
        a.mh_langevin_lineal_propose(k, Ua, out=Pa)
        a.mh_langevin_lineal_accept(k, Ua, Pa, model.forward_device(a, Pa))
        b.mh_langevin_propose(k, Ub, out=Pb)
        b.mh_langevin_accept(k, Ub, Pb, mb.forward_device(b, Pb), DG)
    (sa, _, ca), (sb, _, cb) = a.mh_stats(per_chain=True), b.mh_stats(per_chain=True)
    ua, ub, pa, pb = a.to_host(Ua), b.to_host(Ub), a.mh_phi(), b.mh_phi()
    print("\n[lineal langevin] wide against Jacobian path: accepted %d of %d, max |dU| %.3g max |dphi| %.3g"
          % (ca.sum(), steps * J, np.max(np.abs(ua - ub)), np.max(np.abs(pa - pb))))
    assert sa == sb == steps and np.array_equal(ca, cb) and 0 < ca.sum() < steps * J
    assert np.all(np.abs(ua - ub) <= CAP * (1 + np.abs(ub)))
    assert np.all(np.abs(pa - pb) <= CAP * (1 + np.max(np.abs(pb))))
    a.close()
    b.close()


# ---- 4. the chains against numpy -------------------------------------------------------------------------------------------------

def _sampler(prob, noise="device", dtype="float64", stride=1, seed=None):
    from ces_amd import calibrate, sample
    enka = calibrate.enka(prob["p"], prob["n"], 130)
    enka.Ustar = prob["ens"]
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.engine_dtype, s.trace_stride = True, prob["y"], noise, dtype, stride
    if seed is not None:
        s.seed = seed
    return s, enka, stats.multivariate_normal(mean=prob["mu"], cov=prob["Sigma"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-17x33", (False, False))])
def test_1025_chains_against_numpy(eng_mod, name, forms, dtype):
    """20 steps of 1 025 chains through MCMC.model_mh with injected noise against np_chains_mala_lineal: the caps of
    test_gpu_map_langevin.py::test_1025_chains_against_numpy."""
    prob = lc.problem(name, *forms)
    M, steps, p = 1025, 20, prob["p"]
    s, enka, prior = _sampler(prob, noise="numpy", dtype=dtype, stride=steps)
    np.random.seed(5)
    s.model_mh(lc.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], chains=M, update="langevin")
    assert s.fused_launches == 0
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    Ur, acc = lc.np_chains_mala_lineal(prob, lc.scales(prob), U0, steps, 5)
    rate = acc.sum() / (steps * M)
    Ud = s.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    print("\n[lineal langevin] %s %s: agree %.5f accept device %.6f numpy %.6f" % (name, dtype, agree.mean(), s.accept, rate))
    assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(s.accept - rate) <= (1e-12 if dtype == "float64" else 0.01)
    assert 0.05 < s.accept < 0.999


@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-17x33", (False, False))])
def test_one_chain_equals_the_host_sampler(eng_mod, name, forms):
    """chains=1 on an fp64 engine under one seed: the host sampler's states within 1e-9 (1 + |U|), its accept rate within 1e-12."""
    prob = lc.problem(name, *forms)
    steps, runs = 20, []
    for chains in (dict(chains=1), {}):
        s, enka, prior = _sampler(prob, noise="numpy")
        np.random.seed(13)
        s.model_mh(lc.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], update="langevin", **chains)
        runs.append(s)
    dev, host = runs
    assert dev.samples.shape == host.samples.shape == (prob["p"], steps + 1)
    assert np.all(np.abs(dev.samples - host.samples) <= CAP * (1 + np.abs(host.samples)))
    assert abs(dev.accept - host.accept) <= 1e-12 and 0 < host.accept <= 1


# ---- 5. invariance ------------------------------------------------------------------------------------------------------------------

def test_gaussian_posterior_is_invariant_on_the_device(eng_mod):
    """16 384 chains from exact posterior draws, p = 5, n = 3, 200 steps with device noise, fp64: the z of the mean and of the
    variances of the final states against m and diag C stay within 5."""
    prob = lc.problem("lineal-5x3", False, False)
    M, steps = 16384, 200
    s, enka, prior = _sampler(prob, noise="device", stride=steps)
    enka.Ustar = lc.exact_draws(prob, M, 11)
    s.model_mh(lc.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], chains=M, start="ensemble", update="langevin")
    zm, zv = lc.moment_z(s.samples[:, -1, :], prob["m"], np.diag(prob["C"]))
    print("\n[lineal langevin] invariance on the device: accept %.4f z mean %s z var %s" % (s.accept, zm, zv))
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.5 < s.accept < 0.95


# ---- 6. contracts -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-5x3", (False, True))])
def test_device_noise_bit_identical_and_exact_resume(eng_mod, name, forms):
    """257 chains, device noise: two runs of 12 steps are equal, and 5 + 7 resumed steps end where 12 end."""
    prob = lc.problem(name, *forms)

    def run(splits):
        s, enka, prior = _sampler(prob, noise="device", seed=99)
        enka.Ustar = lc.exact_draws(prob, 257, 4)
        for n in splits:
            s.model_mh(lc.model_of(prob), n, prior, enka, prob["Gamma"], delta=prob["delta"], chains=257, start="ensemble",
                       update="langevin")
            assert s.fused_launches == 0
        return s.samples
    one = run([12])
    assert np.array_equal(one, run([12]))
    two = run([5, 7])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
    assert not np.array_equal(one[:, 0, :], one[:, -1, :])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_shard_reproduces_its_global_columns(eng_mod, dtype):
    """An engine over the columns [33, 98) of J_global = 130 reproduces those columns of the whole-range run bit for bit: U,
    counters, phi and g, after 7 steps with device noise."""
    prob = lc.problem("lineal-17x33", True, True)
    lo, hi, Jg = 33, 98, 130
    U0 = _states(prob, Jg, dtype)
    res = []
    for J, off, cols in ((Jg, 0, slice(None)), (hi - lo, lo, slice(lo, hi))):
        eng, model, U, _ = _started(eng_mod, prob, J, dtype, U0=np.ascontiguousarray(U0[:, cols]), J_global=Jg, j_offset=off)
        P = eng.empty(prob["p"])
        for k in range(7):
            eng.mh_langevin_lineal_propose(k, U, out=P)
            eng.mh_langevin_lineal_accept(k, U, P, model.forward_device(eng, P))
        _, _, per = eng.mh_stats(per_chain=True)
        res.append((eng.to_host(U).copy(), per.copy(), eng.mh_phi(), eng.mh_langevin_lineal_g()))
        eng.close()
    (uw, cw, pw, gw), (us, cs_, ps, gs) = res
    assert np.array_equal(us, uw[:, lo:hi]) and np.array_equal(cs_, cw[lo:hi])
    assert np.array_equal(ps, pw[lo:hi]) and np.array_equal(gs, gw[:, lo:hi]) and 0 < cw.sum() < 7 * Jg


def test_summary_and_marginals_equal_numpy_on_the_trace(eng_mod):
    prob = lc.problem("lineal-5x3", True, False)
    M, steps, p = 257, 24, prob["p"]
    runs = []
    for extra in ({}, dict(summary=True, marginals=True)):
        s, enka, prior = _sampler(prob, noise="device", seed=7)
        enka.Ustar = lc.exact_draws(prob, M, 4)
        s.model_mh(lc.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], chains=M, start="ensemble",
                   update="langevin", **extra)
        runs.append(s)
    tr, sm = runs
    assert np.array_equal(sm.samples[:, -1, :], tr.samples[:, -1, :]) and tr.accept == sm.accept
    draws = cs.draws_of(tr.samples, steps, 1, 0)            # (N, p, M): every state but the start
    assert draws.shape == (steps, p, M)
    ref = cs.ref_raw(draws)
    want, bounds = cs.finalise_ref(ref), cs.summary_bounds(ref)
    assert sm.summary["n"] == steps and sm.summary["chains"] == M
    for k, b in bounds.items():
        assert np.all(np.abs(sm.summary[k] - want[k]) <= b), (k, float(np.max(np.abs(sm.summary[k] - want[k]) / b)))
    mg = sm.marginals
    assert mg["n"] == steps and mg["chains"] == M and mg["hist1d"].sum() > 0
    for r in range(p):
        x = draws[:, r, :].ravel()
        assert np.array_equal(mg["hist1d"][r], np.histogram(x, bins=mg["edges"][r])[0])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("forms", [(False, False), (True, True)], ids=["diagonal", "dense"])
def test_a_nan_column_rejects_that_chain_alone(eng_mod, forms, dtype):
    prob = lc.problem("lineal-17x33", *forms)
    J, bad = 130, 67
    eng, model, U, _ = _started(eng_mod, prob, J, dtype)
    U0, phi0, g0 = eng.to_host(U).copy(), eng.mh_phi().copy(), eng.mh_langevin_lineal_g().copy()
    P = eng.mh_langevin_lineal_propose(0, U)
    GP = model.forward_device(eng, P).clone()
    GP[5, bad] = float("nan")
    eng.mh_langevin_lineal_accept(0, U, P, GP)
    _, _, per = eng.mh_stats(per_chain=True)
    U1, phi1, g1 = eng.to_host(U), eng.mh_phi(), eng.mh_langevin_lineal_g()
    assert per[bad] == 0 and np.array_equal(U1[:, bad], U0[:, bad]) and phi1[bad] == phi0[bad] and np.array_equal(g1[:, bad], g0[:, bad])
    took = per.astype(bool)
    assert 0 < took.sum() < J and np.all(np.isfinite(U1)) and np.all(np.isfinite(g1)) and np.all(np.isfinite(phi1))
    assert np.array_equal(U1[:, took], eng.to_host(P)[:, took]) and np.array_equal(U1[:, ~took], U0[:, ~took])
    assert np.array_equal(g1[:, ~took], g0[:, ~took]) and not np.array_equal(g1[:, took], g0[:, took])
    eng.close()


def test_abi_states_leave_the_chains_untouched(eng_mod):
    """Every ESTATE / EINVAL case of cesx_mh_langevin_lineal_* returns its code, launches nothing and leaves U and cesx_mh_phi
    as they were -- the cross-family refusals and the drop by set_problem / mh_set_proposal included; the run then goes on."""
    import torch
    E = eng_mod
    prob = lc.problem("lineal-5x3", False, True)
    p, n, M = prob["p"], prob["n"], 30
    S = lc.scales(prob)
    model = lc.model_of(prob)
    eng = E.Engine(p, n, M, dtype="float64")
    lib, h = eng.lib, eng._h
    U = eng.to_device(_states(prob, M, "float64"), p, "U").clone()
    P, G = eng.empty(p), eng.empty(n)
    DG = torch.as_tensor(np.ascontiguousarray(np.repeat(prob["A"][:, :, None], M, axis=2)), device=eng.device)
    A = np.ascontiguousarray(prob["A"])
    ptr = lambda t: t.data_ptr()      # noqa: E731
    dp = E._dptr
    lset = lambda a=A, e=0: lib.cesx_mh_langevin_lineal_set(h, None if a is None else dp(a), None, e)      # noqa: E731
    start = lambda: lib.cesx_mh_langevin_lineal_start(h, ptr(U), ptr(G), None)      # noqa: E731
    propose = lambda: lib.cesx_mh_langevin_lineal_propose(h, 0, ptr(U), None, ptr(P), None)      # noqa: E731
    accept = lambda: lib.cesx_mh_langevin_lineal_accept(h, 0, ptr(U), ptr(P), ptr(G), None, None)      # noqa: E731
    gbuf = np.zeros((p, M))
    getg = lambda: lib.cesx_mh_langevin_lineal_g(h, dp(gbuf))      # noqa: E731
    every = lambda: (lset(), start(), propose(), accept(), getg())      # noqa: E731

    # nothing installed: no problem, no proposal
    assert every() == (E.ESTATE,) * 5
    eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["Sigma"], prob["mu"])
    assert every() == (E.ESTATE,) * 5
    eng.mh_set_proposal(None, S)
    assert every() == (E.ESTATE,) * 5                      # a random-walk proposal is no Langevin proposal
    eng.mh_set_proposal("langevin", S)
    assert start() == E.ESTATE and propose() == E.ESTATE and accept() == E.ESTATE and getg() == E.ESTATE      # no set
    assert lset(a=None) == E.EINVAL and lset(e=2) == E.EINVAL
    bad = A.copy()
    bad[1, 2] = np.inf
    assert lset(a=bad) == E.EINVAL
    assert lset() == E.OK
    assert propose() == E.ESTATE and accept() == E.ESTATE and getg() == E.ESTATE      # no start
    for args in ((None, ptr(G)), (ptr(U), None)):
        assert lib.cesx_mh_langevin_lineal_start(h, *args, None) == E.EINVAL
    # the images hold Gamma, Sigma and S: a new problem or proposal drops them
    eng.mh_set_proposal("langevin", S)
    assert start() == E.ESTATE
    assert lset() == E.OK
    eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["Sigma"], prob["mu"])
    eng.mh_set_proposal("langevin", S)
    assert start() == E.ESTATE

    # a started run, then every refusal against its state
    model.langevin_device(eng)
    model.forward_device(eng, U, out=G)
    eng.mh_langevin_lineal_start(U, G)
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert accept() == E.ESTATE                            # no propose since the start
    assert lib.cesx_mh_langevin_lineal_propose(h, 1 << 31, ptr(U), None, ptr(P), None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_propose(h, 0, ptr(U), None, ptr(U), None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_propose(h, 0, None, None, ptr(P), None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_propose(h, 0, ptr(U), None, None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_g(h, None) == E.EINVAL
    # the generic family after a lineal start
    assert lib.cesx_mh_langevin_propose(h, 0, ptr(U), None, ptr(P), None) == E.ESTATE
    assert lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(P), ptr(G), ptr(DG), None, None) == E.ESTATE
    assert lib.cesx_mh_langevin_run_map(h, 0, 3, 1, ptr(U), None, None, None, None) == E.ESTATE
    assert propose() == E.OK
    assert lib.cesx_mh_langevin_lineal_accept(h, 1 << 31, ptr(U), ptr(P), ptr(G), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_accept(h, 0, ptr(U), ptr(U), ptr(G), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_accept(h, 0, None, ptr(P), ptr(G), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_accept(h, 0, ptr(U), None, ptr(G), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_lineal_accept(h, 0, ptr(U), ptr(P), None, None, None) == E.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0)
    steps, rate = eng.mh_stats()
    assert steps == 0 and rate == 0.0
    # and the run goes on
    model.forward_device(eng, P, out=G)
    assert accept() == E.OK and eng.mh_stats()[0] == 1 and getg() == E.OK
    assert accept() == E.ESTATE                            # no propose since the last accept
    # the other way round: after a generic start the lineal family is refused, and a lineal start brings it back
    model.forward_device(eng, U, out=G)
    eng.mh_langevin_start(U, G, DG)
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert propose() == E.ESTATE and accept() == E.ESTATE and getg() == E.ESTATE
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0)
    assert lib.cesx_mh_langevin_propose(h, 0, ptr(U), None, ptr(P), None) == E.OK
    assert start() == E.OK and propose() == E.OK
    model.forward_device(eng, P, out=G)
    assert accept() == E.OK and eng.mh_stats()[0] == 1
    # the wrappers check shape, dtype and contiguity
    with pytest.raises(ValueError, match="contiguous"):
        eng.mh_langevin_lineal_start(U[:, :5], G)
    with pytest.raises(ValueError, match="contiguous"):
        eng.mh_langevin_lineal_propose(0, U.to(torch.float32))
    with pytest.raises(ValueError, match="n_obs, p"):
        eng.mh_langevin_lineal_set(A.T)
    eng.close()
