"""model_mh / gp_mh(chains=M, adapt=) on the device: the adaptation phase (the ADAPT kernels of kernels_hmc.hip and
ad_update_kernel, cesx_mh_adapt_*) against the numpy restatement of tests/adapt_cases.py at the ragged ends of the chain
kernels and of the reduction, the join with the frozen step, chains=1 against the host sampler, what it is for (a step 8 x
too long and one 16 x too short end near the target), and the contracts (summaries, a NaN trajectory, ABI states)."""
import functools
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapt_cases as ac  # noqa: E402
import chain_summary_cases as cs  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402

pytestmark = pytest.mark.gpu

A_STEPS = 12
SIZES = [1, 63, 64, 65, 257, 1023, 1024, 1025, 2049]      # the ragged ends of the 256-thread kernels and of the reduce
# The start steps of the phase tests and of chains=1: 0.75 x lc.DELTA for the maps and 0.05 for the emulator, so that e moves
# from its first step on (to 1.3 .. 1.7 within 12 steps).  Conditions on the inputs, from numpy alone: there the fp64 reference
# and the reference with its positions rounded to fp32 agree within 1e-4 (1 + |U|) on EVERY chain at all nine sizes, both L
# and all five cases.  At other steps the pair itself misses the 0.97 share of the fp32 test -- elliptic at L = 3 agrees on
# 0.29 .. 0.98 of the chains at 2 x lc.DELTA, the emulator's single chain (M = 1) parts at 0.07, 0.08 and 0.1 --: one
# rounding-flipped decision moves abar, through it e by 1e-5 .. 1e-4, and with e every chain.
MAP_FACTOR = 0.75
GP_DELTA = 0.05
CASES = ["elliptic", "banana", "gamma", "var", "gamma_var"]
# fp32 engine: |log ebar_A - the fp32-rounded reference's| over CASES x L x SIZES.  Nothing derives this bound -- a flipped
# decision feeds back through abar --: it is 4 x the worst value the first run on the card measured, 2.106e-05 (banana,
# L = 3, M = 1; the next two 4.97e-06 and 2.94e-06, both single chains; every chain of all 90 cases agreed; NOTEBOOK.md).
FP32_LOG_EBAR_WORST = 2.106e-05
FP32_LOG_EBAR_BOUND = 4 * FP32_LOG_EBAR_WORST


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def _update_kw(L):
    return dict(update="langevin") if L == 1 else dict(update="hmc", leapfrog=L)


def _target(L):
    return ac.TARGET["langevin" if L == 1 else "hmc"]


def _map_sampler(kind, noise="numpy", dtype="float64", seed=1234, particles=130):
    from ces_amd import calibrate, sample
    prob = mc_.problem(kind, None)
    model, y, Gamma, mean, cov, _ = prob
    enka = calibrate.enka(2, 2, particles)
    enka.Ustar = mc_.start_ensemble(kind, particles, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.engine_dtype, s.seed = True, y, noise, dtype, seed
    return s, enka, stats.multivariate_normal(mean=mean, cov=cov), prob


def _gp_kw(a, mode):
    Gamma = None if mode == "var" else a["prob_Gamma_diag"]
    kw = {} if Gamma is None else dict(Gamma=Gamma)
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    return Gamma, kw


def _gp_sampler(a, noise="numpy", dtype="float64", seed=1234):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    mc.engine_dtype, mc.noise, mc.seed = dtype, noise, seed
    return mc


def _run_case(case, L, M, n_mcmc, A, dtype="float64", noise="numpy", seed=1234, **extra):
    """One sampler call on a case of CASES with ``start='mean'``; returns the sampler."""
    if case in ("elliptic", "banana"):
        s, enka, prior, prob = _map_sampler(case, noise, dtype, seed)
        s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], delta=MAP_FACTOR * lc.DELTA[case], chains=M, adapt=A,
                   **_update_kw(L), **extra)
        return s
    man, a = load_gold()
    _, kw = _gp_kw(a, case)
    mc = _gp_sampler(a, noise, dtype, seed)
    mc.gp_mh(gold_problem(a), n_mcmc, gold_prior(a), delta=GP_DELTA, chains=M, adapt=A, **_update_kw(L), **kw, **extra)
    return mc


@functools.lru_cache(maxsize=None)
def _reference(case, L, M, round32):
    """np_adapt on the case under seed 5: (states (A, p, M), history (A, 2), ebar_A), read-only."""
    from ces_amd import calibrate  # noqa: F401  (the cases import the package's host classes)
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if round32 else (lambda x: x)
    if case in ("elliptic", "banana"):
        S = ac.scales(case, MAP_FACTOR)
        U0 = np.repeat(mc_.start_ensemble(case, 130, np.random.default_rng(4)).mean(axis=1)[:, None], M, axis=1)
        score = ac.map_score(case, S)
    else:
        man, a = load_gold()
        enka, prior = gold_problem(a), gold_prior(a)
        Gamma, _ = _gp_kw(a, case)
        S = GP_DELTA * np.linalg.cholesky(np.cov(enka.Ustar))
        U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
        score = ac.gp_score(enka, enka.gpmodels, np.asarray(a["prob_y"]), prior, S, case, Gamma if Gamma is not None else np.eye(4))
    state = np.random.get_state()
    np.random.seed(5)
    states, hist, mult, _ = ac.np_adapt(score, S, U0, A_STEPS, L, _target(L), rnd=rnd)
    np.random.set_state(state)
    states.setflags(write=False)
    hist.setflags(write=False)
    return states, hist, mult


# ---- the adaptation phase against numpy ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_adaptation_phase_against_numpy(eng_mod, case, L, M):
    """fp64 engine, injected noise, A = 12 (then one step at the frozen step).  With d_t the chains whose state after step t
    differs from the reference's by more than 1e-9 (1 + |U|): |abar_t - ref| <= 1e-9 + d_t / M (each alpha lies in [0, 1]),
    the multiplier history within 1e-9 relative up to the first t with d_t > 0, and d_A / M <= 0.001."""
    np.random.seed(5)
    s = _run_case(case, L, M, A_STEPS + 1, A_STEPS)
    states, hist, mult = _reference(case, L, M, False)
    tr = s.samples.reshape(2, A_STEPS + 2, M)
    d = np.array([ac.differing(tr[:, t + 1, :], states[t]).sum() for t in range(A_STEPS)])
    ad = s.adapt
    print("\n[adapt] %s L=%d M=%d: d_A %d multiplier %.6f ref %.6f abar_A %.4f" % (case, L, M, d[-1], ad["multiplier"], mult, hist[-1, 1]))
    assert ad["steps"] == A_STEPS and ad["accept_history"].shape == (A_STEPS,)
    assert np.all(np.abs(ad["accept_history"] - hist[:, 1]) <= 1e-9 + d / M), (ad["accept_history"] - hist[:, 1], d)
    first = int(np.argmax(d > 0)) + 1 if np.any(d > 0) else A_STEPS      # e_t depends on abar_1 .. abar_{t-1}
    assert np.all(np.abs(ad["multiplier_history"][:first] - hist[:first, 0]) <= 1e-9 * hist[:first, 0])
    if not np.any(d > 0):
        assert abs(ad["multiplier"] - mult) <= 1e-9 * mult
    assert d[-1] / M <= 0.001, d
    assert ad["multiplier_history"][0] == 1.0 and ad["multiplier"] != 1.0
    assert ad["delta"] == (MAP_FACTOR * lc.DELTA[case] if case in lc.DELTA else GP_DELTA) * ad["multiplier"]


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_adaptation_phase_fp32_engine(eng_mod, case, L, M):
    """The same cases on an fp32 engine against the reference with its positions rounded to fp32: at least 0.97 of the
    chains agree within 1e-4 (1 + |U|) after the phase (the existing chain tests' share), and log ebar_A is within
    FP32_LOG_EBAR_BOUND of the reference's."""
    np.random.seed(5)
    s = _run_case(case, L, M, A_STEPS + 1, A_STEPS, dtype="float32")
    states, hist, mult = _reference(case, L, M, True)
    tr = s.samples.reshape(2, A_STEPS + 2, M)
    agree = 1.0 - ac.differing(tr[:, A_STEPS, :], states[-1], cap=1e-4).mean()
    err = abs(np.log(s.adapt["multiplier"]) - np.log(mult))
    print("\n[adapt fp32] %s L=%d M=%d: agree %.5f |log ebar_A - ref| %.3e" % (case, L, M, agree, err))
    assert agree >= 0.97, agree
    assert err <= FP32_LOG_EBAR_BOUND, err


# ---- the join -------------------------------------------------------------------------------------------------------------------

def _join_run(case, fused, adapt, n_mcmc, resume_from=None):
    M = 257
    if case == "gp":
        man, a = load_gold()
        s = _gp_sampler(a, noise="device", seed=99)
        # (the gold ensemble has 30 particles: 257 chains start at its mean; the device noise differs per chain)
        call = lambda delta, **kw: s.gp_mh(gold_problem(a), n_mcmc, gold_prior(a), delta=delta, chains=M, update="hmc",      # noqa: E731
                                           leapfrog=2, Gamma=a["prob_Gamma_diag"], **kw)
        delta = 3 * GP_DELTA
    else:
        s, enka, prior, prob = _map_sampler(case, noise="device", seed=99, particles=M)
        call = lambda delta, **kw: s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], delta=delta, chains=M, start="ensemble",      # noqa: E731
                                              update="hmc", leapfrog=2, fused=fused, **kw)
        delta = MAP_FACTOR * lc.DELTA[case]
    if resume_from is not None:
        s.samples, s._mh_next_step, delta = resume_from.samples[:, :adapt + 1, :].copy(), adapt, resume_from.adapt["delta"]
        call(delta)
    else:
        call(delta, adapt=adapt)
    return s


@pytest.mark.parametrize("case, fused", [("elliptic", True), ("elliptic", False), ("gp", None)],
                         ids=["elliptic-fused", "elliptic-step", "emulator"])
def test_the_join_is_exact(eng_mod, case, fused):
    """Run X: ``adapt=8`` of 20 steps, device noise, 257 chains.  Run Y: a fresh sampler resumed from X's trace up to step 8 at
    ``delta = X.adapt['delta']`` for 12 steps without ``adapt``.  Equal final states bit for bit, equal ``accept``; two X runs
    are equal bit for bit."""
    X = _join_run(case, fused, 8, 20)
    X2 = _join_run(case, fused, 8, 20)
    assert np.array_equal(X.samples, X2.samples) and X.accept == X2.accept
    assert X.adapt["multiplier"] == X2.adapt["multiplier"] and np.array_equal(X.adapt["accept_history"], X2.adapt["accept_history"])
    assert X.samples.shape == (2, 21, 257) and (X.fused_launches > 0) == bool(fused)
    Y = _join_run(case, fused, 8, 12, resume_from=X)
    assert not hasattr(Y, "adapt")
    assert np.array_equal(Y.samples[:, -1, :], X.samples[:, -1, :])
    assert np.array_equal(Y.samples, X.samples)
    assert X.accept == Y.accept and np.array_equal(X.accept_chains, Y.accept_chains)
    assert 0 < X.accept < 1 and X.adapt["multiplier"] != 1.0


# ---- chains=1 against the host sampler -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("case", ["elliptic", "banana", "gamma", "var"])
def test_one_chain_is_the_host_sampler(eng_mod, case, L):
    """``chains=1`` with injected noise and the host sampler under one seed, ``adapt=10`` of 24 steps: states and ``self.adapt``
    within 1e-9 (1 + |x|)."""
    from test_map_langevin_host import _quiet_banana
    A, n = 10, 24
    np.random.seed(8)
    dev = _run_case(case, L, 1, n, A)
    np.random.seed(8)
    if case in ("elliptic", "banana"):
        host, enka, prior, prob = _map_sampler(case)
        model = _quiet_banana() if case == "banana" else prob[0]
        host.model_mh(model, n, prior, enka, prob[2], delta=MAP_FACTOR * lc.DELTA[case], adapt=A, **_update_kw(L))
    else:
        man, a = load_gold()
        _, kw = _gp_kw(a, case)
        host = _gp_sampler(a)
        host.gp_mh(gold_problem(a), n, gold_prior(a), delta=GP_DELTA, adapt=A, **_update_kw(L), **kw)
    close = lambda x, y: bool(np.all(np.abs(np.asarray(x) - np.asarray(y)) <= 1e-9 * (1 + np.abs(np.asarray(y)))))      # noqa: E731
    assert dev.samples.shape == host.samples.shape == (2, n + 1)
    assert close(dev.samples, host.samples)
    for k in ("multiplier", "delta", "accept_history", "multiplier_history"):
        assert close(dev.adapt[k], host.adapt[k]), k
    assert dev.adapt["steps"] == host.adapt["steps"] == A and dev.adapt["target"] == host.adapt["target"]
    assert dev.accept == pytest.approx(host.accept, abs=1e-12)


# ---- what it is for --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which, factor", [("long", 8.0), ("short", 1.0 / 16.0)])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_a_wrong_step_ends_near_the_target(eng_mod, kind, L, which, factor):
    """1 024 chains from the start ensemble, device noise, delta 8 x too long and 16 x too short (the factors the numpy
    reference converged from, test_adapt_host.py), A = 100, then 100 steps: ``accept`` within 0.05 of the target (twice the
    reference's band), the multiplier below 1 / 4 or above 4."""
    M = 1024
    s, enka, prior, prob = _map_sampler(kind, noise="device", seed=17, particles=M)
    s.trace_stride = 100
    s.model_mh(prob[0], 200, prior, enka, prob[2], delta=factor * lc.DELTA[kind], chains=M, start="ensemble", adapt=100,
               **_update_kw(L))
    print("\n[adapt] %s L=%d %s: multiplier %.4f accept %.4f target %.3f" % (kind, L, which, s.adapt["multiplier"], s.accept, _target(L)))
    assert abs(s.accept - _target(L)) <= 0.05, (s.accept, _target(L))
    assert s.adapt["multiplier"] < 0.25 if which == "long" else s.adapt["multiplier"] > 4.0
    assert s.samples.shape == (2, 3, M)


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("mode", ["var", "gamma", "gamma_var"])
def test_a_long_step_on_the_emulator_ends_near_the_target(eng_mod, mode, L):
    """The gold emulator at delta = 0.8, 8 x the Langevin step of test_gpu_gp_langevin.py, 1 024 chains, device noise, A = 100,
    then 100 steps: ``accept`` within 0.05 of the target in the three likelihoods.  The multiplier is below 1 / 4 for
    Sigma = diag(gvars), gp_mh's likelihood without ``Gamma``: there the numpy reference (256 chains, tests/adapt_cases.py)
    finds 0.109 (L = 1) and 0.095 (L = 4).  With Gamma the step 0.1 is shorter than the posterior wants (it accepts up to
    0.95), so 0.8 is less than 8 x too long: the reference itself finds 0.247 / 0.224 (Gamma) and 0.278 / 0.249
    (diag(Gamma) + diag(gvars)), on either side of 1 / 4 -- no property of the rule; those modes keep the acceptance band."""
    man, a = load_gold()
    _, kw = _gp_kw(a, mode)
    mc = _gp_sampler(a, noise="device", seed=17)
    mc.trace_stride = 100
    mc.gp_mh(gold_problem(a), 200, gold_prior(a), delta=0.8, chains=1024, adapt=100, **_update_kw(L), **kw)
    print("\n[adapt] emulator %s L=%d: multiplier %.4f accept %.4f target %.3f" % (mode, L, mc.adapt["multiplier"], mc.accept, _target(L)))
    assert abs(mc.accept - _target(L)) <= 0.05, (mc.accept, _target(L))
    if mode == "var":
        assert mc.adapt["multiplier"] < 0.25


# ---- contracts -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
def test_summary_and_marginals_equal_numpy_on_the_trace(eng_mod, fused):
    """``summary=True, marginals=True, burn=A`` against numpy on the trace of the same run without them
    (test_gpu_hmc.py's pattern): the draws are the states after the steps A + 1 .. n."""
    M, steps, A = 257, 32, 8
    runs = []
    for extra in ({}, dict(summary=True, marginals=True, burn=A)):
        s, enka, prior, prob = _map_sampler("banana", noise="device", seed=7, particles=M)
        s.model_mh(prob[0], steps, prior, enka, prob[2], delta=MAP_FACTOR * lc.DELTA["banana"], chains=M, start="ensemble",
                   update="hmc", leapfrog=2, fused=fused, adapt=A, **extra)
        runs.append(s)
    tr, sm = runs
    assert np.array_equal(sm.samples[:, -1, :], tr.samples[:, -1, :]) and tr.accept == sm.accept
    assert tr.adapt["multiplier"] == sm.adapt["multiplier"]
    draws = cs.draws_of(tr.samples, steps, 1, A)
    assert draws.shape == (steps - A, 2, M)
    ref = cs.ref_raw(draws)
    want, bounds = cs.finalise_ref(ref), cs.summary_bounds(ref)
    assert sm.summary["n"] == steps - A and sm.summary["chains"] == M
    for k, b in bounds.items():
        assert np.all(np.abs(sm.summary[k] - want[k]) <= b), (k, float(np.max(np.abs(sm.summary[k] - want[k]) / b)))
    mg = sm.marginals
    assert mg["n"] == steps - A and mg["chains"] == M and mg["hist1d"].sum() > 0
    for r in range(2):
        assert np.array_equal(mg["hist1d"][r], np.histogram(draws[:, r, :].ravel(), bins=mg["edges"][r])[0])


def _armed_engine(eng_mod, kind, J, A, target, J_global=None, arm=True):
    """An engine with the problem, the Langevin proposal at MAP_FACTOR x the case's step, the map and the start states scored,
    armed for A adaptation steps: (eng, model, U, out, S, U0)."""
    model, y, Gamma, mean, cov, _ = mc_.problem(kind, None)
    eng = eng_mod.Engine(2, 2, J, dtype="float64", J_global=J_global, seed=77)
    eng.set_problem(y, Gamma, mean, cov, mean)
    S = ac.scales(kind, MAP_FACTOR)
    eng.mh_set_proposal("hmc", S)
    if arm:
        eng.mh_adapt_set(A, target)
    U0 = mc_.start_ensemble(kind, J, np.random.default_rng(9))
    U = eng.to_device(U0, 2, "U0").clone()
    out = model.jacobian_device(eng, U)
    eng.mh_langevin_start(U, *out)
    return eng, model, U, out, S, U0


def test_a_nan_trajectory_has_alpha_zero_and_rejects_alone(eng_mod):
    """65 chains, L = 3, A = 4, injected noise.  In step 2 chain 7's column of G is NaN at the second leapfrog (a leap), in
    step 3 chain 40's at the last (the accept): that chain's alpha is 0 and it alone stays; the other chains, abar_t and the
    multiplier match the reference, whose phi and g of that chain are NaN at that position."""
    import torch
    J, L, A = 65, 3, 4
    hits = {(2, 2): 7, (3, 3): 40}
    eng, model, U, out, S, U0 = _armed_engine(eng_mod, "banana", J, A, 0.651)
    np.random.seed(13)
    draws = [(np.random.normal(0, 1, [2, J]), np.log(np.random.uniform(size=J))) for _ in range(A)]
    Q, kept = eng.empty(2), []
    for t in range(1, A + 1):
        xi, logu = draws[t - 1]
        eng.mh_hmc_begin(t - 1, U, xi=eng.to_device(xi, 2, "xi"), out=Q)
        for l in range(1, L + 1):
            model.jacobian_device(eng, Q, out=out)
            if (t, l) in hits:
                out[0][:, hits[(t, l)]] = float("nan")
            if l < L:
                eng.mh_hmc_leap(Q, *out)
            else:
                eng.mh_hmc_accept(t - 1, U, Q, *out, logu=torch.as_tensor(logu, dtype=torch.float64, device=eng.device))
        kept.append(eng.to_host(U).copy())
    got = eng.mh_adapt_read()
    eng.close()

    def poison(t, l, phq, gq):
        if (t, l) in hits:
            phq[hits[(t, l)]] = np.nan
            gq[:, hits[(t, l)]] = np.nan
    np.random.seed(13)
    states, hist, mult, alphas = ac.np_adapt(ac.map_score("banana", S), S, U0, A, L, 0.651, poison=poison)
    assert alphas[1, 7] == 0.0 and alphas[2, 40] == 0.0
    assert np.array_equal(kept[1][:, 7], kept[0][:, 7]) and np.array_equal(kept[2][:, 40], kept[1][:, 40])
    for t in range(A):
        assert not np.any(ac.differing(kept[t], states[t])), t
    assert got["steps"] == A and got["history"].shape == (A, 2)
    assert np.all(np.abs(got["history"] - hist) <= 1e-9 * (1 + np.abs(hist))), got["history"] - hist
    assert abs(got["multiplier"] - mult) <= 1e-9 * mult
    assert np.all(np.isfinite(got["history"]))
    assert 0 < np.sum([not np.array_equal(kept[t], kept[t - 1]) for t in range(1, A)])      # (chains did move)


def test_abi_states_leave_the_chains_untouched(eng_mod):
    """Every CESX_EINVAL / CESX_EUNSUPPORTED / CESX_ESTATE case of cesx_mh_adapt_* and of the calls an armed handle refuses
    returns its code, launches nothing and leaves U and cesx_mh_phi as they were; after the last adaptation step the leapfrog
    calls return CESX_ESTATE; after cesx_mh_set_proposal the unarmed HMC path runs again."""
    import torch
    import ctypes as C
    E = eng_mod
    kind, M, A = "elliptic", 30, 2
    model, y, Gamma, mean, cov, _ = mc_.problem(kind, None)
    S = ac.scales(kind, 1.0)
    eng = E.Engine(2, 2, M, dtype="float64")
    lib, h = eng.lib, eng._h
    aset = lambda n=A, target=0.651, gain=2.0, kappa=0.75: lib.cesx_mh_adapt_set(h, n, target, gain, kappa)      # noqa: E731
    mult, done = C.c_double(0.0), C.c_int32(0)
    aread = lambda: lib.cesx_mh_adapt_read(h, C.byref(mult), C.byref(done), None)      # noqa: E731
    # no problem, no proposal, a random-walk proposal: ESTATE (valid arguments), and nothing to read
    assert aset() == E.ESTATE and aread() == E.ESTATE
    eng.set_problem(y, Gamma, mean, cov, mean)
    assert aset() == E.ESTATE
    eng.mh_set_proposal(None, S)
    assert aset() == E.ESTATE and aread() == E.ESTATE
    eng.mh_set_proposal("hmc", S)
    assert aread() == E.ESTATE                             # not armed
    for bad in (dict(n=0), dict(n=-1), dict(n=ac.STEPS_MAX + 1), dict(target=0.0), dict(target=1.0), dict(target=float("nan")),
                dict(gain=0.0), dict(gain=-1.0), dict(gain=float("nan")), dict(kappa=0.5), dict(kappa=1.01), dict(kappa=float("nan"))):
        assert aset(**bad) == E.EINVAL, bad
    assert aread() == E.ESTATE                             # (none of those armed it)
    assert lib.cesx_mh_adapt_read(h, None, C.byref(done), None) == E.EINVAL

    U = eng.to_device(mc_.start_ensemble(kind, M, np.random.default_rng(0)), 2, "U").clone()
    Q, P = eng.empty(2), eng.empty(2)
    G = torch.zeros((2, M), dtype=torch.float64, device=eng.device)
    DG = torch.zeros((2, 2, M), dtype=torch.float64, device=eng.device)
    model.jacobian_device(eng, U, out=(G, DG))
    eng.mh_langevin_start(U, G, DG)
    assert aset(n=ac.STEPS_MAX) == E.OK and aset() == E.OK      # the largest count arms; re-arming starts over
    assert aread() == E.OK and done.value == 0 and mult.value == 1.0
    torch.cuda.synchronize()
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    ptr = lambda t: t.data_ptr()      # noqa: E731
    # while armed: the fused launches, the single Langevin steps and the lineal family are refused
    assert lib.cesx_mh_hmc_run_map(h, 0, 3, 2, 1, ptr(U), None, None, None, None) == E.ESTATE
    assert lib.cesx_mh_langevin_run_map(h, 0, 3, 1, ptr(U), None, None, None, None) == E.ESTATE
    assert lib.cesx_mh_langevin_propose(h, 0, ptr(U), None, ptr(P), None) == E.ESTATE
    assert lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(P), ptr(G), ptr(DG), None, None) == E.ESTATE
    assert lib.cesx_gp_langevin_propose(h, 0, ptr(U), None, ptr(P), None) == E.ESTATE
    assert lib.cesx_gp_langevin_accept(h, 0, 0, ptr(U), ptr(P), ptr(G), None, ptr(DG), None, None, None) == E.ESTATE
    A2 = np.eye(2)
    assert lib.cesx_mh_langevin_lineal_set(h, A2.ctypes.data_as(C.POINTER(C.c_double)), None, 0) == E.ESTATE
    assert lib.cesx_mh_langevin_lineal_start(h, ptr(U), ptr(G), None) == E.ESTATE
    assert lib.cesx_mh_langevin_lineal_propose(h, 0, ptr(U), None, ptr(P), None) == E.ESTATE
    assert lib.cesx_mh_langevin_lineal_accept(h, 0, ptr(U), ptr(P), ptr(G), None, None) == E.ESTATE
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0) and eng.mh_stats()[0] == 0
    assert aread() == E.OK and done.value == 0

    # the A = 2 adaptation steps of L = 2, then the leapfrog calls are refused: read, then set the proposal
    for step in range(A):
        eng.mh_hmc_begin(step, U, out=Q)
        model.jacobian_device(eng, Q, out=(G, DG))
        eng.mh_hmc_leap(Q, G, DG)
        model.jacobian_device(eng, Q, out=(G, DG))
        eng.mh_hmc_accept(step, U, Q, G, DG)
    torch.cuda.synchronize()
    U1, phi1 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert lib.cesx_mh_hmc_begin(h, A, ptr(U), None, ptr(Q), None) == E.ESTATE
    assert lib.cesx_mh_hmc_leap(h, ptr(Q), ptr(G), ptr(DG), None) == E.ESTATE
    assert lib.cesx_mh_hmc_accept(h, A, ptr(U), ptr(Q), ptr(G), ptr(DG), None, None) == E.ESTATE
    assert lib.cesx_gp_hmc_leap(h, 0, ptr(Q), ptr(G), None, ptr(DG), None, None) == E.ESTATE
    assert lib.cesx_gp_hmc_accept(h, 0, A, ptr(U), ptr(Q), ptr(G), None, ptr(DG), None, None, None) == E.ESTATE
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U1) and np.array_equal(eng.mh_phi(), phi1) and eng.mh_stats()[0] == A
    got = eng.mh_adapt_read()
    assert got["steps"] == A and got["history"].shape == (A, 2) and got["history"][0, 0] == 1.0
    assert np.all((got["history"][:, 1] >= 0) & (got["history"][:, 1] <= 1)) and got["multiplier"] > 0

    # cesx_mh_set_proposal disarms: nothing to read, and the unarmed HMC path and the fused launch run again
    eng.mh_set_proposal("hmc", S)
    assert aread() == E.ESTATE
    model.jacobian_device(eng, U, out=(G, DG))
    eng.mh_langevin_start(U, G, DG)
    eng.mh_hmc_begin(0, U, out=Q)
    model.jacobian_device(eng, Q, out=(G, DG))
    eng.mh_hmc_accept(0, U, Q, G, DG)
    eng.mh_hmc_run_map(1, 3, 2, U)
    assert eng.mh_stats()[0] == 4
    # cesx_set_problem disarms too (another problem: the binding skips the call for the one it holds)
    assert aset() == E.OK
    eng.set_problem(y + 1.0, Gamma, mean, cov, mean)
    assert aread() == E.ESTATE
    eng.close()

    # a shard: pooling across ranks is out of scope
    sh = E.Engine(2, 2, M, dtype="float64", J_global=2 * M, j_offset=0)
    sh.set_problem(y, Gamma, mean, cov, mean)
    sh.mh_set_proposal("hmc", S)
    assert sh.lib.cesx_mh_adapt_set(sh._h, A, 0.651, 2.0, 0.75) == E.EUNSUPPORTED
    assert sh.lib.cesx_mh_adapt_read(sh._h, C.byref(mult), C.byref(done), None) == E.ESTATE
    sh.close()
