"""model_mh / gp_mh(chains=M, update='hmc') on the device: the step path (cesx_mh_hmc_*, cesx_gp_hmc_*) against the vectorised
numpy chains, ``leapfrog=1`` against the Langevin step this repository already has, the fused kernel (cesx_mh_hmc_run_map)
against the step path, and the sampler's contracts (alternation with Langevin steps, chunking, an oversized step, device
noise, resume, shards, fp32, invariance, summaries, ABI states).  Cases, references and bounds: tests/hmc_cases.py on
tests/map_cases.py, tests/map_langevin_cases.py and tests/gp_langevin_cases.py."""
import functools
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_summary_cases as cs  # noqa: E402
import hmc_cases as hc  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402

pytestmark = pytest.mark.gpu

K_STEPS = 7
CAP = 1e-9                                                 # states within CAP (1 + |U|): test_gpu_map_langevin.py's cap


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


_ENGINES = {}


def _sampler(kind, M, noise="device", dtype="float64", stride=1, seed=None, share=True):
    """An MCMC object, its enka (130 particles near the posterior's bulk) and the prior; samplers of one (M, dtype) share one
    engine, so a fused run follows a step-path run on the same handle (test_gpu_map_langevin.py's)."""
    from ces_amd import calibrate, sample
    prob = mc_.problem(kind, None)
    model, y, Gamma, mean, cov, _ = prob
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble(kind, 130, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.engine_dtype, s.trace_stride = True, y, noise, dtype, stride
    if seed is not None:
        s.seed = seed
    if share:
        key = (2, 2, M, dtype, int(s.device), int(s.seed))
        if key not in _ENGINES:
            _ENGINES[key] = s._mh_engine(2, 2, M)
        s._mh_eng, s._mh_key = _ENGINES[key], key
    return s, enka, stats.multivariate_normal(mean=mean, cov=cov), prob


def _under_cap(a, b):
    return bool(np.all(np.abs(a - b) <= CAP * (1 + np.abs(b))))


# ---- the step path against numpy -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _np_map_reference(kind, L, M, steps):
    from ces_amd import calibrate  # noqa: F401  (the cases import the package's host classes)
    U0 = np.repeat(mc_.start_ensemble(kind, 130, np.random.default_rng(4)).mean(axis=1)[:, None], M, axis=1)
    Ur, acc = hc.np_chains_hmc(kind, lc.scales(kind), U0, steps, L, 5)
    Ur.setflags(write=False)
    return Ur, acc.sum() / (steps * M)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_1025_chains_against_numpy(eng_mod, kind, L, dtype):
    """The step path with injected noise against np_chains_hmc, with the caps of
    test_gpu_map_langevin.py::test_1025_chains_against_numpy."""
    M, steps = 1025, 20
    s, enka, prior, prob = _sampler(kind, M, noise="numpy", dtype=dtype, stride=steps)
    np.random.seed(5)
    s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA[kind], chains=M, update="hmc", leapfrog=L, fused=False)
    assert s.fused_launches == 0
    Ur, rate = _np_map_reference(kind, L, M, steps)
    Ud = s.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    print("\n[hmc] %s L=%d %s: agree %.5f accept device %.6f numpy %.6f" % (kind, L, dtype, agree.mean(), s.accept, rate))
    assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(s.accept - rate) <= (1e-12 if dtype == "float64" else 0.01)
    assert 0.05 < s.accept < 0.999


# ---- L = 1 against the Langevin step -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_one_leapfrog_is_the_langevin_step(eng_mod, kind, M, fused):
    """``update='hmc', leapfrog=1`` and ``update='langevin'`` from one seed with device noise, fp64, 12 steps: equal states,
    equal per-chain counters, equal mh_phi(); then ONE single Langevin step on each handle leaves equal states again, which
    pins the g the HMC run left.  (A decision could flip only through the rounding of r = (xi - g / 2) - g' / 2 against
    xi - (g + g') / 2, within a few ulps of the test's two sides.)"""
    import torch
    steps, ends = 12, []
    for kw in (dict(update="hmc", leapfrog=1), dict(update="langevin")):
        s, enka, prior, prob = _sampler(kind, M, seed=31, share=False)
        if M > 130:                                        # (start='ensemble' needs M particles; S is theirs for both runs)
            enka.Ustar = mc_.start_ensemble(kind, M, np.random.default_rng(4))
        s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA[kind], chains=M, start="ensemble", fused=fused, **kw)
        assert (s.fused_launches > 0) == fused
        eng, U = s._mh_eng, s.samples_device
        _, _, per = eng.mh_stats(per_chain=True)
        mid = (eng.to_host(U).copy(), per.copy(), eng.mh_phi().copy())
        P = eng.empty(2)
        eng.mh_langevin_propose(steps, U, out=P)
        out = prob[0].jacobian_device(eng, P)
        eng.mh_langevin_accept(steps, U, P, *out)
        torch.cuda.synchronize()
        _, _, per = eng.mh_stats(per_chain=True)
        ends.append(mid + (eng.to_host(U).copy(), per.copy(), eng.mh_phi().copy()))
        eng.close()
    names = ("states", "counters", "phi", "states after a Langevin step", "counters after it", "phi after it")
    for name, a, b in zip(names, *ends):
        assert np.array_equal(a, b), (name, float(np.max(np.abs(a.astype(np.float64) - b))))
    if M >= 63:
        assert 0 < ends[0][1].sum() < steps * M


# ---- the fused kernel against the step path -----------------------------------------------------------------------------------

def _run(kind, M, fused, n_mcmc, stride, L, start_step=0):
    s, enka, prior, prob = _sampler(kind, M, stride=stride)
    kw = dict(chains=M, start="ensemble", delta=lc.DELTA[kind], update="hmc", leapfrog=L)
    if start_step:                                         # the resume path: the first leg on the step path for both
        s.model_mh(prob[0], start_step, prior, enka, prob[2], fused=False, **kw)
        assert s._mh_next_step == start_step
    first = 0 if not start_step else s.samples.shape[1]
    s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], fused=fused, **kw)
    assert s.fused_launches == (1 if fused else 0)
    samples = s.samples.reshape(2, s.samples.shape[1], M)
    return s, samples[:, first:, :], np.rint(np.asarray(s.accept_chains) * n_mcmc).astype(np.int64), prob


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_fused_equals_the_step_path(eng_mod, kind, M, L):
    """Same seed, device noise, K = 7 steps, stride 1 and 3, from step 0 and from step 5 through the resume path: equal shapes,
    equal per-chain counters, states within 1e-9 (1 + |U|); mh_phi() after the fused run is the fp64 numpy phi of the final
    states within 32 2^-52 sum|terms|; mh_stats reports K steps.  (Elliptic has a diagonal Gamma, banana a dense one, both a
    dense prior; the diagonal prior: test_fused_single_hmc_and_single_langevin_steps_alternate.)"""
    for stride in (1, 3):
        for start_step in (0, 5):
            _, a, ca, _ = _run(kind, M, False, K_STEPS, stride, L, start_step)
            s, b, cb, prob = _run(kind, M, True, K_STEPS, stride, L, start_step)
            case = (stride, start_step)
            assert a.shape == b.shape == (2, (0 if start_step else 1) + K_STEPS // stride + (1 if K_STEPS % stride else 0), M), case
            assert np.array_equal(ca, cb), case
            if stride == 1 and start_step == 0 and M >= 63:
                assert 0 < ca.sum() < K_STEPS * M
            assert _under_cap(b, a), case
            final = np.ascontiguousarray(b[:, -1, :])
            assert np.array_equal(s.samples_device.cpu().numpy(), final)
            phi, mag = mc_.phi_numpy(prob, final)
            got = s._mh_eng.mh_phi()
            assert np.all(np.abs(got - phi) <= 32 * 2.0 ** -52 * mag), (case, float(np.max(np.abs(got - phi) / mag)))
            steps, _, per = s._mh_eng.mh_stats(per_chain=True)
            assert steps == K_STEPS and np.array_equal(per.astype(np.int64), cb)


def _prepared_engine(eng_mod, kind, J, dtype="float64", J_global=None, j_offset=0, cols=None, diag_prior=False, delta=None,
                     seed=77, rng=9):
    """An engine with the problem, the Langevin proposal, the model's map and the start states scored: (eng, model, U, out)."""
    prob = mc_.problem(kind, None)
    model, y, Gamma, mean, cov, _ = prob
    if diag_prior:
        cov = np.diag(np.diag(cov))
    eng = eng_mod.Engine(2, 2, J, dtype=dtype, J_global=J_global, j_offset=j_offset, seed=seed)
    eng.set_problem(y, Gamma, mean, cov, mean)
    eng.mh_set_proposal("hmc", lc.scales(kind) if delta is None else lc.scales(kind) * (delta / lc.DELTA[kind]))
    U0 = mc_.start_ensemble(kind, J_global or J, np.random.default_rng(rng)).astype(np.float32).astype(np.float64)
    if cols is not None:
        U0 = np.ascontiguousarray(U0[:, cols])
    U = eng.to_device(U0, 2, "U0").clone()
    out = model.jacobian_device(eng, U)
    eng.mh_langevin_start(U, *out)
    return eng, model, U, out


def _single_hmc(eng, model, U, Q, out, step, L):
    eng.mh_hmc_begin(step, U, out=Q)
    for _ in range(L - 1):
        model.jacobian_device(eng, Q, out=out)
        eng.mh_hmc_leap(Q, *out)
    model.jacobian_device(eng, Q, out=out)
    eng.mh_hmc_accept(step, U, Q, *out)


def _single_langevin(eng, model, U, P, out, step):
    eng.mh_langevin_propose(step, U, out=P)
    model.jacobian_device(eng, P, out=out)
    eng.mh_langevin_accept(step, U, P, *out)


@pytest.mark.parametrize("kind, diag_prior", [("elliptic", False), ("elliptic", True), ("banana", True)],
                         ids=["elliptic", "elliptic-diag-prior", "banana-diag-prior"])
def test_fused_single_hmc_and_single_langevin_steps_alternate(eng_mod, kind, diag_prior):
    """3 fused HMC steps (L = 3), one single HMC step, one single Langevin step, 2 fused Langevin steps, 2 fused HMC steps
    (L = 2): equal to the same nine steps all on the step path, with equal counters -- phi and g are handed over every way.
    With a diagonal prior covariance too, which the sampler's cases do not reach."""
    import torch
    J = 65
    ends = []
    for mixed in (False, True):
        eng, model, U, out = _prepared_engine(eng_mod, kind, J, diag_prior=diag_prior)
        P = eng.empty(2)
        if mixed:
            eng.mh_hmc_run_map(0, 3, 3, U)
            _single_hmc(eng, model, U, P, out, 3, 3)
            _single_langevin(eng, model, U, P, out, 4)
            eng.mh_langevin_run_map(5, 2, U)
            eng.mh_hmc_run_map(7, 2, 2, U)
        else:
            for step in range(4):
                _single_hmc(eng, model, U, P, out, step, 3)
            for step in range(4, 7):
                _single_langevin(eng, model, U, P, out, step)
            for step in range(7, 9):
                _single_hmc(eng, model, U, P, out, step, 2)
        steps, _, per = eng.mh_stats(per_chain=True)
        assert steps == 9
        torch.cuda.synchronize()
        ends.append((U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (Ua, ca, pa), (Ub, cb, pb) = ends
    assert np.array_equal(ca, cb) and 0 < ca.sum() < 9 * J
    assert _under_cap(Ub, Ua)
    assert np.allclose(pa, pb, rtol=0.0, atol=1e-9 * (1 + np.max(np.abs(pa))))


def test_a_long_run_is_chunked(eng_mod):
    """700 steps of L = 8 at 65 chains are 5 600 gradient evaluations: two fused launches (512 + 188 steps), and the result
    equals the step path's under the cap.  A launch of 4 097 evaluations is refused with CESX_EINVAL and launches nothing."""
    M, steps, L = 65, 700, 8
    res = []
    for fused, stride in ((False, 4), (True, 4), (True, steps)):      # (a stride longer than a launch: still two launches)
        s, enka, prior, prob = _sampler("elliptic", M, stride=stride, seed=3)
        s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA["elliptic"], chains=M, start="ensemble", update="hmc",
                   leapfrog=L, fused=fused)
        assert s.fused_launches == (2 if fused else 0)
        assert s.samples.shape == (2, 1 + steps // stride, M)
        res.append((s.samples, np.asarray(s.accept_chains)))
    assert np.array_equal(res[0][1], res[1][1]) and _under_cap(res[1][0], res[0][0])
    assert np.array_equal(res[0][1], res[2][1]) and _under_cap(res[2][0][:, -1, :], res[0][0][:, -1, :])
    eng, model, U, _ = _prepared_engine(eng_mod, "elliptic", M)
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    for n, lf in ((4097, 1), (241, 17), (65, 64)):
        assert n * lf > hc.GRADS_MAX
        assert eng.lib.cesx_mh_hmc_run_map(eng._h, 0, n, lf, 1, U.data_ptr(), None, None, None, None) == eng_mod.EINVAL
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0) and eng.mh_stats()[0] == 0
    eng.mh_hmc_run_map(0, 64, 64, U)                       # 4 096 exactly: runs
    assert eng.mh_stats()[0] == 64
    eng.close()


@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
def test_an_oversized_step_rejects_everything(eng_mod, fused):
    """Elliptic at delta = 42, L = 4, 257 chains, 6 steps: every trajectory leaves the posterior's bulk so far that exp
    overflows or the energy error is astronomical -- plain IEEE arithmetic, numpy gives the same --, so accept is 0, the
    final states are the start states bit for bit and everything is finite."""
    import torch
    J = 257
    eng, model, U, out = _prepared_engine(eng_mod, "elliptic", J, delta=42.0)
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    if fused:
        eng.mh_hmc_run_map(0, 6, 4, U)
    else:
        Q = eng.empty(2)
        for step in range(6):
            _single_hmc(eng, model, U, Q, out, step, 4)
    torch.cuda.synchronize()
    steps, rate, per = eng.mh_stats(per_chain=True)
    assert steps == 6 and rate == 0.0 and per.sum() == 0
    assert np.array_equal(eng.to_host(U), U0) and np.all(np.isfinite(U0))
    assert np.array_equal(eng.mh_phi(), phi0) and np.all(np.isfinite(phi0))
    eng.close()


# ---- device noise ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [False, True, None], ids=["step", "fused", "default"])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_device_noise_bit_identical_and_exact_resume(eng_mod, kind, fused):
    """257 chains, device noise, L = 3: two runs of 12 steps are equal, and 5 + 7 resumed steps end where 12 end -- on the step
    path and fused (the resume scores the resumed states through the Langevin start, and g enters the next trajectory: the
    fused kernel has to leave the step path's g bit for bit).  ``fused=None`` is ``LANGEVIN_FUSED_DEFAULT``."""
    from ces_amd import sample

    def run(splits):
        s, enka, prior, prob = _sampler(kind, 257, noise="device", seed=99, share=False)
        enka.Ustar = mc_.start_ensemble(kind, 257, np.random.default_rng(4))
        for n in splits:
            s.model_mh(prob[0], n, prior, enka, prob[2], delta=lc.DELTA[kind], chains=257, start="ensemble",
                       update="hmc", leapfrog=3, fused=fused)
            want = sample.MCMC.LANGEVIN_FUSED_DEFAULT if fused is None else fused
            assert (s.fused_launches > 0) == bool(want)
        return s.samples
    one = run([12])
    assert np.array_equal(one, run([12]))
    two = run([5, 7])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
    assert not np.array_equal(one[:, 0, :], one[:, -1, :])


def test_a_step_consumes_one_step_index_whatever_L_is(eng_mod):
    """The xi block of step 3 is the Langevin step's: the first position of an HMC step equals cesx_mh_langevin_propose's P bit
    for bit, at L = 1 and at L = 5 (begin does not know L)."""
    J = 65
    eng, model, U, out = _prepared_engine(eng_mod, "banana", J)
    P, Q = eng.empty(2), eng.empty(2)
    eng.mh_langevin_propose(3, U, out=P)
    eng.mh_hmc_begin(3, U, out=Q)
    assert np.array_equal(eng.to_host(P), eng.to_host(Q)) and not np.array_equal(eng.to_host(Q), eng.to_host(U))
    eng.close()


def test_fp32_engine_is_the_fp64_launch_rounded_on_the_store(eng_mod):
    """One fused launch (K = 7, L = 3, device noise, the same seed) on an fp32 and on an fp64 engine from start states exactly
    representable in fp32: the fp32 trace and final U are the fp64 ones cast to float32 bit for bit, the counters equal."""
    import torch
    J = 65
    for kind in ("elliptic", "banana"):
        res = {}
        for dtype in ("float32", "float64"):
            eng, model, U, _ = _prepared_engine(eng_mod, kind, J, dtype=dtype)
            trace = torch.empty((K_STEPS, 2, J), dtype=eng.torch_dtype, device=eng.device)
            eng.mh_hmc_run_map(3, K_STEPS, 3, U, stride=1, trace=trace)
            _, _, per = eng.mh_stats(per_chain=True)
            res[dtype] = (trace.cpu().numpy(), U.cpu().numpy(), per.copy())
            eng.close()
        t32, u32, c32 = res["float32"]
        t64, u64, c64 = res["float64"]
        assert t32.dtype == np.float32 and t64.dtype == np.float64
        assert np.array_equal(c32, c64) and 0 < c64.sum() < K_STEPS * J
        assert np.array_equal(t32, t64.astype(np.float32)) and np.array_equal(u32, u64.astype(np.float32))
        assert np.array_equal(t64[-1], u64)


@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
def test_a_shard_draws_the_noise_of_its_global_columns(eng_mod, fused):
    """An engine over the columns [33, 98) of J_global = 130 reproduces those columns of the whole-range run bit for bit."""
    import torch
    lo, hi, Jg, L = 33, 98, 130, 3
    res = []
    for J, off, cols in ((Jg, 0, None), (hi - lo, lo, slice(lo, hi))):
        eng, model, U, out = _prepared_engine(eng_mod, "banana", J, J_global=Jg, j_offset=off, cols=cols)
        if fused:
            trace = torch.empty((K_STEPS // 3, 2, J), dtype=eng.torch_dtype, device=eng.device)
            eng.mh_hmc_run_map(0, K_STEPS, L, U, stride=3, trace=trace)
            tr = trace.cpu().numpy()
        else:
            Q = eng.empty(2)
            for step in range(K_STEPS):
                _single_hmc(eng, model, U, Q, out, step, L)
            tr = np.zeros((0, 2, J))
        _, _, per = eng.mh_stats(per_chain=True)
        res.append((tr, U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (tw, uw, cw, pw), (ts, us, cs_, ps) = res
    assert np.array_equal(ts, tw[:, :, lo:hi]) and np.array_equal(us, uw[:, lo:hi])
    assert np.array_equal(cs_, cw[lo:hi]) and np.array_equal(ps, pw[lo:hi]) and cw.sum() > 0


@pytest.fixture(scope="module")
def quadrature():
    return lc.banana_quadrature()


def test_banana_posterior_is_invariant_on_the_device(eng_mod, quadrature):
    """16 384 chains from the start ensemble, 400 fused steps of L = 4 at ``scales('banana')`` with device noise, one launch
    (1 600 gradient evaluations): mean and second central moments of the final states within 5 standard errors of the
    quadrature of exp(-phi); accept in (0.55, 0.67) (numpy: 0.607)."""
    import torch
    mean, var = quadrature
    M, steps, L = 16384, 400, 4
    prob = mc_.problem("banana", None)
    model, y, Gamma, pm, cov, _ = prob
    eng = eng_mod.Engine(2, 2, M, dtype="float64", seed=5)
    eng.set_problem(y, Gamma, pm, cov, pm)
    eng.mh_set_proposal("hmc", lc.scales("banana"))
    U = eng.to_device(mc_.start_ensemble("banana", M, np.random.default_rng(4)), 2, "U0").clone()
    eng.mh_langevin_start(U, *model.jacobian_device(eng, U))
    eng.mh_hmc_run_map(0, steps, L, U)
    torch.cuda.synchronize()
    n, rate = eng.mh_stats()
    zm, zv = lc.moment_z(eng.to_host(U), mean, var)
    print("\n[hmc] banana invariance on the device: accept %.4f z mean %s z var %s" % (rate, zm, zv))
    eng.close()
    assert n == steps
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.55 < rate < 0.67


@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
def test_summary_and_marginals_equal_numpy_on_the_trace(eng_mod, fused):
    M, steps = 257, 24
    runs = []
    for extra in ({}, dict(summary=True, marginals=True)):
        s, enka, prior, prob = _sampler("banana", M, noise="device", seed=7, share=False)
        enka.Ustar = mc_.start_ensemble("banana", M, np.random.default_rng(4))
        s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA["banana"], chains=M, start="ensemble", update="hmc",
                   leapfrog=2, fused=fused, **extra)
        runs.append(s)
    tr, sm = runs
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


# ---- the emulator ---------------------------------------------------------------------------------------------------------------

# The emulator's step.  At test_gpu_gp_langevin.py's 0.1 the likelihood diag(gvars) at L = 3 accepts 0.28 and its trajectories
# are sensitive: the numpy chain with its positions rounded to fp32 (what an fp32 engine stores) agrees with the fp64 numpy chain
# within 1e-4 (1 + |U|) on 0.923 of the chains only -- the reference alone misses the fp32 cap of 0.97.  At 0.07 numpy against
# rounded numpy agrees on 100 % of the chains in all three modes at L = 1 and 3, and numpy accepts 0.72 .. 0.98.
GP_DELTA = 0.07


def _gp_kw(a, mode):
    Gamma = None if mode == "var" else a["prob_Gamma_diag"]
    kw = {} if Gamma is None else dict(Gamma=Gamma)
    if mode == "gamma_var":
        kw["noise_compounded"] = True
    return Gamma, kw


def _gp_mcmc(a, dtype="float64", noise="numpy", seed=1234, stride=1):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    mc.engine_dtype, mc.noise, mc.seed, mc.trace_stride = dtype, noise, seed, stride
    return mc


@functools.lru_cache(maxsize=None)
def _np_gp_reference(mode, L, M, steps):
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    Gamma, _ = _gp_kw(a, mode)
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    scales = GP_DELTA * np.linalg.cholesky(np.cov(enka.Ustar))
    Ur, rate = hc.np_chains_hmc_gp(enka, enka.gpmodels, a["prob_y"], prior, scales, U0, steps, L, mode,
                                   Gamma if Gamma is not None else np.eye(4), True, 5)
    Ur.setflags(write=False)
    return Ur, rate.mean()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var"])
def test_emulator_1024_chains_against_numpy(mode, L, dtype):
    """gp_mh(chains=1 024, update='hmc') with injected noise against np_chains_hmc_gp, with the caps of
    test_gpu_gp_langevin.py::test_1024_chains_against_numpy."""
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    _, kw = _gp_kw(a, mode)
    M, steps = 1024, 20
    mc = _gp_mcmc(a, dtype, stride=steps)
    np.random.seed(5)
    mc.gp_mh(enka, steps, prior, delta=GP_DELTA, chains=M, update="hmc", leapfrog=L, **kw)
    assert mc.fused_launches == 0
    Ur, rate = _np_gp_reference(mode, L, M, steps)
    Ud = mc.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    print("\n[hmc] emulator %s L=%d %s: agree %.5f accept device %.6f numpy %.6f" % (mode, L, dtype, agree.mean(), mc.accept, rate))
    assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(mc.accept - rate) <= (1e-12 if dtype == "float64" else 0.01)
    assert 0.05 < mc.accept < 0.999


@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var"])
def test_emulator_one_leapfrog_is_the_langevin_step(mode):
    """gp_mh(update='hmc', leapfrog=1) and gp_mh(update='langevin'), one seed, device noise, fp64, 257 chains, 12 steps and a
    resumed 3: equal states, equal per-chain rates."""
    man, a = load_gold()
    _, kw = _gp_kw(a, mode)
    ends = []
    for upd in (dict(update="hmc", leapfrog=1), dict(update="langevin")):
        mc = _gp_mcmc(a, noise="device", seed=99)
        for n in (12, 3):
            mc.gp_mh(gold_problem(a), n, gold_prior(a), delta=GP_DELTA, chains=257, **upd, **kw)
        ends.append((mc.samples, mc.accept_chains, mc._mh_eng.mh_phi()))
    for x, y in zip(*ends):
        assert np.array_equal(x, y)
    assert not np.array_equal(ends[0][0][:, 0, :], ends[0][0][:, -1, :])


def test_emulator_device_noise_bit_identical_and_exact_resume():
    man, a = load_gold()

    def run(splits):
        enka = gold_problem(a)
        mc = _gp_mcmc(a, noise="device", seed=99)
        for s in splits:
            mc.gp_mh(enka, s, gold_prior(a), delta=GP_DELTA, chains=257, update="hmc", leapfrog=3)
        return mc.samples
    one = run([12])
    assert np.array_equal(one, run([12]))
    two = run([5, 7])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
    assert not np.array_equal(one[:, 0, :], one[:, -1, :])


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

def test_abi_states_leave_the_chains_untouched(eng_mod):
    """Every ESTATE / EINVAL case of cesx_mh_hmc_*, cesx_gp_hmc_* and cesx_mh_hmc_run_map returns its code, launches nothing and
    leaves U, cesx_mh_phi, g and the counters as they were; the run then goes on."""
    import torch
    from ces_amd import utils
    E = eng_mod
    kind, M = "elliptic", 30
    model, y, Gamma, mean, cov, _ = mc_.problem(kind, None)
    eng = E.Engine(2, 2, M, dtype="float64")
    lib, h = eng.lib, eng._h
    U = eng.to_device(mc_.start_ensemble(kind, M, np.random.default_rng(0)), 2, "U").clone()
    Q = eng.empty(2)
    G = torch.zeros((2, M), dtype=torch.float64, device=eng.device)
    DG = torch.zeros((2, 2, M), dtype=torch.float64, device=eng.device)
    ptr = lambda t: t.data_ptr()      # noqa: E731
    begin = lambda step=0: lib.cesx_mh_hmc_begin(h, step, ptr(U), None, ptr(Q), None)      # noqa: E731
    leap = lambda: lib.cesx_mh_hmc_leap(h, ptr(Q), ptr(G), ptr(DG), None)      # noqa: E731
    accept = lambda step=0: lib.cesx_mh_hmc_accept(h, step, ptr(U), ptr(Q), ptr(G), ptr(DG), None, None)      # noqa: E731
    gp_leap = lambda: lib.cesx_gp_hmc_leap(h, 0, ptr(Q), ptr(G), None, ptr(DG), None, None)      # noqa: E731
    gp_accept = lambda: lib.cesx_gp_hmc_accept(h, 0, 0, ptr(U), ptr(Q), ptr(G), None, ptr(DG), None, None, None)      # noqa: E731
    run = lambda step=1, n=3, lf=2, stride=1: lib.cesx_mh_hmc_run_map(h, step, n, lf, stride, ptr(U), None, None, None, None)      # noqa: E731
    S = lc.scales(kind)

    # nothing installed: no problem, no proposal, no start
    assert begin() == E.ESTATE and leap() == E.ESTATE and accept() == E.ESTATE and run() == E.ESTATE
    assert gp_leap() == E.ESTATE and gp_accept() == E.ESTATE
    eng.set_problem(y, Gamma, mean, cov, mean)
    eng.mh_set_proposal(None, S)
    assert begin() == E.ESTATE and run() == E.ESTATE       # a random-walk proposal is no Langevin proposal
    eng.mh_set_proposal("hmc", S)
    assert begin() == E.ESTATE and leap() == E.ESTATE and accept() == E.ESTATE and run() == E.ESTATE      # no start

    # a linear-map start is no start for a leapfrog
    lin = utils.lineal(np.array([[1.0, 0.5], [0.2, 1.0]]))
    lin.enable_gradient()
    lin.langevin_device(eng)
    Gl = lin.forward_device(eng, U)
    eng.mh_langevin_lineal_start(U, Gl)
    assert begin() == E.ESTATE and run() == E.ESTATE

    # a started run, then every refusal against its state
    model.jacobian_device(eng, U, out=(G, DG))
    eng.mh_langevin_start(U, G, DG)
    torch.cuda.synchronize()
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert leap() == E.ESTATE and accept() == E.ESTATE     # no begin since the start
    assert gp_leap() == E.ESTATE and gp_accept() == E.ESTATE
    eng.map_set("exp")
    assert run() == E.ESTATE                               # installed, but no fused kind
    model.ensure_installed(eng)
    assert begin(1 << 31) == E.EINVAL
    assert lib.cesx_mh_hmc_begin(h, 0, ptr(U), None, ptr(U), None) == E.EINVAL
    assert lib.cesx_mh_hmc_begin(h, 0, None, None, ptr(Q), None) == E.EINVAL
    assert lib.cesx_mh_hmc_begin(h, 0, ptr(U), None, None, None) == E.EINVAL
    assert leap() == E.ESTATE                              # (none of those began a trajectory)
    assert begin() == E.OK
    assert gp_leap() == E.ESTATE and gp_accept() == E.ESTATE      # begun, but no emulator
    for args in ((None, ptr(G), ptr(DG)), (ptr(Q), None, ptr(DG)), (ptr(Q), ptr(G), None)):
        assert lib.cesx_mh_hmc_leap(h, *args, None) == E.EINVAL
    assert accept(1 << 31) == E.EINVAL
    assert lib.cesx_mh_hmc_accept(h, 0, ptr(U), ptr(U), ptr(G), ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_hmc_accept(h, 0, None, ptr(Q), ptr(G), ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_hmc_accept(h, 0, ptr(U), None, ptr(G), ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_hmc_accept(h, 0, ptr(U), ptr(Q), None, ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_hmc_accept(h, 0, ptr(U), ptr(Q), ptr(G), None, None, None) == E.EINVAL
    assert run(n=0) == E.EINVAL and run(stride=0) == E.EINVAL and run(lf=0) == E.EINVAL and run(lf=65) == E.EINVAL and run(lf=-1) == E.EINVAL
    assert run(n=2049, lf=2) == E.EINVAL
    assert run(step=2 ** 31 - 2) == E.EINVAL and run(step=1 << 31) == E.EINVAL
    assert lib.cesx_mh_hmc_run_map(h, 0, 3, 2, 1, None, None, None, None, None) == E.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0)
    steps, rate = eng.mh_stats()
    assert steps == 0 and rate == 0.0
    # a Langevin propose takes the noise block over: the trajectory in flight is gone, and the other way round
    P = eng.empty(2)
    eng.mh_langevin_propose(0, U, out=P)
    assert leap() == E.ESTATE and accept() == E.ESTATE
    assert begin() == E.OK
    assert lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(P), ptr(G), ptr(DG), None, None) == E.ESTATE
    # and the run goes on: one whole step of L = 2, then a fused launch; the g the refusals left is the start's
    model.jacobian_device(eng, Q, out=(G, DG))
    assert leap() == E.OK
    model.jacobian_device(eng, Q, out=(G, DG))
    assert accept() == E.OK
    assert leap() == E.ESTATE                              # the accept ended the trajectory
    assert eng.mh_stats()[0] == 1
    assert run() == E.OK
    assert eng.mh_stats()[0] == 4
    torch.cuda.synchronize()
    Ua, ca = eng.to_host(U).copy(), eng.mh_stats(per_chain=True)[2].copy()
    eng.close()
    # the same four steps on a fresh handle that saw no refusal
    eng = E.Engine(2, 2, M, dtype="float64")
    eng.set_problem(y, Gamma, mean, cov, mean)
    eng.mh_set_proposal("hmc", S)
    U = eng.to_device(U0, 2, "U").clone()
    out = model.jacobian_device(eng, U)
    eng.mh_langevin_start(U, *out)
    _single_hmc(eng, model, U, eng.empty(2), out, 0, 2)
    eng.mh_hmc_run_map(1, 3, 2, U)
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), Ua) and np.array_equal(eng.mh_stats(per_chain=True)[2], ca)
    eng.close()
