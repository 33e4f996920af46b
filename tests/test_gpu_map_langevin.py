"""model_mh(chains=M, update='langevin') on the device: cesx_map_jac against the host Jacobians, the step path
(cesx_mh_langevin_*) against the vectorised numpy chains, the fused kernel (cesx_mh_langevin_run_map) against the step path, and
the sampler's contracts (alternation, injected noise, fp32, shards, invariance, resume, summaries, ABI states).  Cases,
references and bounds: tests/map_cases.py, tests/map_langevin_cases.py."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_summary_cases as cs  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = mc_.EPS
K_STEPS = 7
CAP = 1e-9                                                 # states within CAP (1 + |U|): the issue's cap of the fused comparison


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


# ---- cesx_map_jac ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("J", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_map_jac_against_the_host_class(eng_mod, kind, J, dtype):
    """G is what map_apply forms before it rounds (fp64 engine: equal; fp32 engine: map_apply's is G rounded), and
    |DG_dev - DG_host| <= 8 2^-52 sum|terms| per entry at the U the engine holds (1 ulp for ocml's exp, the rounding of each
    operation).  An ``out=`` call writes into the tensors given."""
    import torch
    from ces_amd import utils
    model = utils.elliptic() if kind == "elliptic" else utils.banana(a=1.3, b=0.4)
    U = mc_.as_engine(mc_.draw_U(kind, J, np.random.default_rng(J)), dtype)
    eng = eng_mod.Engine(2, 2, J, dtype=dtype)
    Ud = eng.to_device(U, 2, "U")
    G, DG = model.jacobian_device(eng, Ud)
    assert G.dtype == DG.dtype == torch.float64 and tuple(G.shape) == (2, J) and tuple(DG.shape) == (2, 2, J)
    Ga = model.forward_device(eng, Ud).cpu().numpy()
    assert np.array_equal(Ga, G.cpu().numpy().astype(eng.np_dtype))
    want, bound = model.jacobian(U), 8 * EPS["float64"] * lc.jac_abs_terms(model, U)
    err = np.abs(DG.cpu().numpy() - want)
    print("\n[map langevin] jac %s J=%d %s: worst err / bound %.3g" % (kind, J, dtype, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(err <= bound)
    out = (torch.zeros_like(G), torch.zeros_like(DG))
    got = model.jacobian_device(eng, Ud, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], G) and torch.equal(out[1], DG)
    eng.close()


# ---- the samplers ---------------------------------------------------------------------------------------------------------

_ENGINES = {}


def _sampler(kind, M, noise="device", dtype="float64", stride=1, seed=None, share=True):
    """An MCMC object, its enka (130 particles near the posterior's bulk) and the prior; samplers of one (M, dtype) share one
    engine, so a fused run follows a step-path run on the same handle."""
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


def _run(kind, M, fused, n_mcmc, stride, start_step=0, noise="device", seed=None):
    s, enka, prior, prob = _sampler(kind, M, noise=noise, stride=stride)
    kw = dict(chains=M, start="ensemble", delta=lc.DELTA[kind], update="langevin")
    if seed is not None:
        np.random.seed(seed)
    if start_step:                                         # the resume path: the first leg on the step path for both
        s.model_mh(prob[0], start_step, prior, enka, prob[2], fused=False, **kw)
        assert s._mh_next_step == start_step
    first = 0 if not start_step else s.samples.shape[1]
    s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], fused=fused, **kw)
    assert s.fused_launches == (1 if fused else 0)
    samples = s.samples.reshape(2, s.samples.shape[1], M)
    return s, samples[:, first:, :], np.rint(np.asarray(s.accept_chains) * n_mcmc).astype(np.int64), prob


def _under_cap(a, b):
    return bool(np.all(np.abs(a - b) <= CAP * (1 + np.abs(b))))


def _ulps(a, b):
    """The worst error as a multiple of test_gpu_maps._bound = 4 K 2^-52 max(1, max|U|) (reported, not asserted: the gradient
    amplifies a rounding of the state by |S S^T Hess phi|, which that bound does not know)."""
    return float(np.max(np.abs(a - b))) / (4 * K_STEPS * 2.0 ** -52 * max(1.0, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_1025_chains_against_numpy(eng_mod, kind, dtype):
    """The step path with injected noise against np_chains_mala: the caps of
    test_gpu_gp_langevin.py::test_1024_chains_against_numpy."""
    M, steps = 1025, 20
    s, enka, prior, prob = _sampler(kind, M, noise="numpy", dtype=dtype, stride=steps)
    np.random.seed(5)
    s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA[kind], chains=M, update="langevin", fused=False)
    assert s.fused_launches == 0
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    Ur, acc = lc.np_chains_mala(kind, lc.scales(kind), U0, steps, 5)
    rate = acc.sum() / (steps * M)
    Ud = s.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    print("\n[map langevin] %s %s: agree %.5f accept device %.6f numpy %.6f" % (kind, dtype, agree.mean(), s.accept, rate))
    assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(s.accept - rate) <= (1e-12 if dtype == "float64" else 0.01)
    assert 0.05 < s.accept < 0.999


@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_fused_equals_the_step_path(eng_mod, kind, M):
    """Same seed, device noise, K = 7 steps, stride 1 and 3, from step 0 and from step 5 through the resume path: equal shapes,
    equal per-chain counters, states within 1e-9 (1 + |U|); mh_phi() after the fused run is the fp64 numpy phi of the final
    states within 32 2^-52 sum|terms|; mh_stats reports K steps."""
    worst = 0.0
    for stride in (1, 3):
        for start_step in (0, 5):
            _, a, ca, _ = _run(kind, M, False, K_STEPS, stride, start_step)
            s, b, cb, prob = _run(kind, M, True, K_STEPS, stride, start_step)
            case = (stride, start_step)
            assert a.shape == b.shape == (2, (0 if start_step else 1) + K_STEPS // stride + (1 if K_STEPS % stride else 0), M), case
            assert np.array_equal(ca, cb), case
            if stride == 1 and start_step == 0 and M >= 63:
                assert 0 < ca.sum() < K_STEPS * M
            worst = max(worst, _ulps(b, a))
            assert _under_cap(b, a), case
            final = np.ascontiguousarray(b[:, -1, :])
            assert np.array_equal(s.samples_device.cpu().numpy(), final)
            phi, mag = mc_.phi_numpy(prob, final)
            got = s._mh_eng.mh_phi()
            assert np.all(np.abs(got - phi) <= 32 * 2.0 ** -52 * mag), (case, float(np.max(np.abs(got - phi) / mag)))
            steps, _, per = s._mh_eng.mh_stats(per_chain=True)
            assert steps == K_STEPS and np.array_equal(per.astype(np.int64), cb)
    print("\n[map langevin] fused vs step %s M=%d: worst err %.3g x 4 K 2^-52 max(1, |U|)" % (kind, M, worst))


def _prepared_engine(eng_mod, kind, J, dtype="float64", J_global=None, j_offset=0, cols=None, diag_prior=False):
    """An engine with the problem, the Langevin proposal, the model's map and the start states scored: (eng, model, U, out)."""
    prob = mc_.problem(kind, None)
    model, y, Gamma, mean, cov, _ = prob
    if diag_prior:
        cov = np.diag(np.diag(cov))
    eng = eng_mod.Engine(2, 2, J, dtype=dtype, J_global=J_global, j_offset=j_offset, seed=77)
    eng.set_problem(y, Gamma, mean, cov, mean)
    eng.mh_set_proposal("langevin", lc.scales(kind))
    U0 = mc_.start_ensemble(kind, J_global or J, np.random.default_rng(9)).astype(np.float32).astype(np.float64)
    if cols is not None:
        U0 = np.ascontiguousarray(U0[:, cols])
    U = eng.to_device(U0, 2, "U0").clone()
    out = model.jacobian_device(eng, U)
    eng.mh_langevin_start(U, *out)
    return eng, model, U, out


@pytest.mark.parametrize("kind, diag_prior", [("elliptic", False), ("elliptic", True), ("banana", True)],
                         ids=["elliptic", "elliptic-diag-prior", "banana-diag-prior"])
def test_fused_launches_and_single_steps_alternate(eng_mod, kind, diag_prior):
    """A 4-step fused launch, one single step (jacobian_device, propose, accept), 2 more fused steps: equal to 7 single steps
    with equal counters -- the chains' g is handed over both ways.  With a diagonal prior covariance too, which the sampler's
    cases (the random walk's dense one) do not reach: the kernel's forms for a diagonal Sigma, with either Gamma."""
    import torch
    J = 65
    ends = []
    for mixed in (False, True):
        eng, model, U, out = _prepared_engine(eng_mod, kind, J, diag_prior=diag_prior)
        P = eng.empty(2)

        def single(step):
            eng.mh_langevin_propose(step, U, out=P)
            model.jacobian_device(eng, P, out=out)
            eng.mh_langevin_accept(step, U, P, *out)
        if mixed:
            eng.mh_langevin_run_map(0, 4, U)
            single(4)
            eng.mh_langevin_run_map(5, 2, U)
        else:
            for step in range(7):
                single(step)
        steps, _, per = eng.mh_stats(per_chain=True)
        assert steps == 7
        torch.cuda.synchronize()
        ends.append((U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (Ua, ca, pa), (Ub, cb, pb) = ends
    assert np.array_equal(ca, cb) and 0 < ca.sum() < 7 * J
    print("\n[map langevin] alternation %s diag_prior=%s: worst err %.3g x 4 K 2^-52 max(1, |U|)" % (kind, diag_prior, _ulps(Ub, Ua)))
    assert _under_cap(Ub, Ua)
    assert np.allclose(pa, pb, rtol=0.0, atol=1e-9 * (1 + np.max(np.abs(pa))))


@pytest.mark.parametrize("M", [1, 65])
def test_fused_with_injected_noise(eng_mod, M):
    """``noise='numpy'`` under one np.random.seed: fused=True equals fused=False (counters equal, states under the cap); for
    M = 1 it is also the host ``model_mh(update='langevin')`` under the same seed (elliptic: the host banana class draws from
    the global RNG in every call)."""
    from ces_amd import sample
    n_mcmc = K_STEPS
    for kind in ("elliptic", "banana"):
        _, a, ca, _ = _run(kind, M, False, n_mcmc, 1, noise="numpy", seed=11)
        s, b, cb, prob = _run(kind, M, True, n_mcmc, 1, noise="numpy", seed=11)
        assert s.samples.shape == ((2, n_mcmc + 1) if M == 1 else (2, n_mcmc + 1, M))
        assert np.array_equal(ca, cb) and _under_cap(b, a)
    if M == 1:
        s, enka, prior, prob = _sampler("elliptic", 1, noise="numpy")
        kw = dict(delta=lc.DELTA["elliptic"], update="langevin")
        np.random.seed(5)
        s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], chains=1, fused=True, **kw)
        host = sample.MCMC()
        host.mute_bar, host.y_obs = True, prob[1]
        np.random.seed(5)
        host.model_mh(prob[0], n_mcmc, prior, enka, prob[2], **kw)
        assert s.samples.shape == host.samples.shape == (2, n_mcmc + 1)
        assert _under_cap(s.samples, host.samples)
        assert s.accept == pytest.approx(host.accept, abs=1e-12)


def test_fp32_engine_is_the_fp64_launch_rounded_on_the_store(eng_mod):
    """One fused launch (K = 7, device noise, the same seed) on an fp32 and on an fp64 engine from start states exactly
    representable in fp32: the fp32 trace and final U are the fp64 ones cast to float32 bit for bit, the counters equal."""
    import torch
    J = 65
    for kind in ("elliptic", "banana"):
        res = {}
        for dtype in ("float32", "float64"):
            eng, model, U, _ = _prepared_engine(eng_mod, kind, J, dtype=dtype)
            trace = torch.empty((K_STEPS, 2, J), dtype=eng.torch_dtype, device=eng.device)
            eng.mh_langevin_run_map(3, K_STEPS, U, stride=1, trace=trace)
            _, _, per = eng.mh_stats(per_chain=True)
            res[dtype] = (trace.cpu().numpy(), U.cpu().numpy(), per.copy())
            eng.close()
        t32, u32, c32 = res["float32"]
        t64, u64, c64 = res["float64"]
        assert t32.dtype == np.float32 and t64.dtype == np.float64
        assert np.array_equal(c32, c64) and 0 < c64.sum() < K_STEPS * J
        assert np.array_equal(t32, t64.astype(np.float32)) and np.array_equal(u32, u64.astype(np.float32))
        assert np.array_equal(t64[-1], u64)


def test_a_shard_draws_the_noise_of_its_global_columns(eng_mod):
    """An engine over the columns [33, 98) of J_global = 130 reproduces those columns of the whole-range fused run bit for
    bit: trace, U, counters and phi."""
    import torch
    lo, hi, Jg = 33, 98, 130
    res = []
    for J, off, cols in ((Jg, 0, None), (hi - lo, lo, slice(lo, hi))):
        eng, model, U, _ = _prepared_engine(eng_mod, "banana", J, J_global=Jg, j_offset=off, cols=cols)
        trace = torch.empty((K_STEPS // 3, 2, J), dtype=eng.torch_dtype, device=eng.device)
        eng.mh_langevin_run_map(0, K_STEPS, U, stride=3, trace=trace)
        _, _, per = eng.mh_stats(per_chain=True)
        res.append((trace.cpu().numpy(), U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (tw, uw, cw, pw), (ts, us, cs_, ps) = res
    assert np.array_equal(ts, tw[:, :, lo:hi]) and np.array_equal(us, uw[:, lo:hi])
    assert np.array_equal(cs_, cw[lo:hi]) and np.array_equal(ps, pw[lo:hi]) and cw.sum() > 0


@pytest.fixture(scope="module")
def quadrature():
    return lc.banana_quadrature()


def test_banana_posterior_is_invariant_on_the_device(eng_mod, quadrature):
    """16 384 chains from the start ensemble, 400 fused steps with device noise: mean and second central moments of the final
    states within 5 standard errors of the quadrature of exp(-phi); accept rate as numpy's 0.679."""
    mean, var = quadrature
    M, steps = 16384, 400
    s, enka, prior, prob = _sampler("banana", M, noise="device", stride=steps, share=False)
    enka.Ustar = mc_.start_ensemble("banana", M, np.random.default_rng(4))
    s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA["banana"], chains=M, start="ensemble", update="langevin",
               fused=True)
    zm, zv = lc.moment_z(s.samples[:, -1, :], mean, var)
    print("\n[map langevin] banana invariance on the device: accept %.4f z mean %s z var %s" % (s.accept, zm, zv))
    assert s.fused_launches == 1
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.6 < s.accept < 0.75


@pytest.mark.parametrize("fused", [False, True, None], ids=["step", "fused", "default"])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_device_noise_bit_identical_and_exact_resume(eng_mod, kind, fused):
    """257 chains, device noise: two runs of 12 steps are equal, and 5 + 7 resumed steps end where 12 end -- on the step path
    and fused (the resume scores the resumed states with the step path's kernel, and g enters the next proposal: the fused
    kernel has to leave the step path's g bit for bit).  ``fused=None`` is ``LANGEVIN_FUSED_DEFAULT``."""
    from ces_amd import sample

    def run(splits):
        s, enka, prior, prob = _sampler(kind, 257, noise="device", seed=99, share=False)
        enka.Ustar = mc_.start_ensemble(kind, 257, np.random.default_rng(4))
        for n in splits:
            s.model_mh(prob[0], n, prior, enka, prob[2], delta=lc.DELTA[kind], chains=257, start="ensemble",
                       update="langevin", fused=fused)
            want = sample.MCMC.LANGEVIN_FUSED_DEFAULT if fused is None else fused
            assert (s.fused_launches > 0) == bool(want)
        return s.samples
    one = run([12])
    assert np.array_equal(one, run([12]))
    two = run([5, 7])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
    assert not np.array_equal(one[:, 0, :], one[:, -1, :])


@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
def test_summary_and_marginals_equal_numpy_on_the_trace(eng_mod, fused):
    M, steps = 257, 24
    runs = []
    for extra in ({}, dict(summary=True, marginals=True)):
        s, enka, prior, prob = _sampler("banana", M, noise="device", seed=7, share=False)
        enka.Ustar = mc_.start_ensemble("banana", M, np.random.default_rng(4))
        s.model_mh(prob[0], steps, prior, enka, prob[2], delta=lc.DELTA["banana"], chains=M, start="ensemble", update="langevin",
                   fused=fused, **extra)
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


def test_abi_states_leave_the_chains_untouched(eng_mod):
    """Every ESTATE / EINVAL / EUNSUPPORTED case of cesx_map_jac, cesx_mh_langevin_* and cesx_mh_langevin_run_map returns its
    code, launches nothing and leaves U and cesx_mh_phi as they were; the run then goes on."""
    import torch
    from ces_amd import utils
    E = eng_mod
    kind, M = "elliptic", 30
    model, y, Gamma, mean, cov, _ = mc_.problem(kind, None)
    eng = E.Engine(2, 2, M, dtype="float64")
    lib, h = eng.lib, eng._h
    U = eng.to_device(mc_.start_ensemble(kind, M, np.random.default_rng(0)), 2, "U").clone()
    P = eng.empty(2)
    G = torch.zeros((2, M), dtype=torch.float64, device=eng.device)
    DG = torch.zeros((2, 2, M), dtype=torch.float64, device=eng.device)
    ptr = lambda t: t.data_ptr()      # noqa: E731
    jac = lambda: lib.cesx_map_jac(h, ptr(U), ptr(G), ptr(DG), None)      # noqa: E731
    start = lambda: lib.cesx_mh_langevin_start(h, ptr(U), ptr(G), ptr(DG), None)      # noqa: E731
    propose = lambda: lib.cesx_mh_langevin_propose(h, 0, ptr(U), None, ptr(P), None)      # noqa: E731
    accept = lambda: lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(P), ptr(G), ptr(DG), None, None)      # noqa: E731
    run = lambda step=1, n=3, stride=1: lib.cesx_mh_langevin_run_map(h, step, n, stride, ptr(U), None, None, None, None)      # noqa: E731
    S = lc.scales(kind)

    # nothing installed: no problem, no proposal, no map
    assert jac() == E.ESTATE
    assert start() == E.ESTATE and propose() == E.ESTATE and accept() == E.ESTATE and run() == E.ESTATE
    eng.set_problem(y, Gamma, mean, cov, mean)
    assert start() == E.ESTATE                             # no proposal
    eng.mh_set_proposal(None, S)
    assert start() == E.ESTATE and run() == E.ESTATE       # a random-walk proposal is no Langevin proposal
    eng.mh_set_proposal("langevin", S)
    assert propose() == E.ESTATE and accept() == E.ESTATE and run() == E.ESTATE      # no start
    assert jac() == E.ESTATE                               # still no map
    eng.map_set("exp")
    assert jac() == E.EUNSUPPORTED
    with pytest.raises(E.CesxError) as exc:
        eng.map_jac(U, out=(G, DG))
    assert exc.value.code == E.EUNSUPPORTED
    for args in ((None, ptr(G), ptr(DG)), (ptr(U), None, ptr(DG)), (ptr(U), ptr(G), None)):
        assert lib.cesx_map_jac(h, *args, None) == E.EINVAL
        assert lib.cesx_mh_langevin_start(h, *args, None) == E.EINVAL

    # a started run, then every refusal against its state
    eng.map_set("exp")                                     # (another model's map: this one installs itself again)
    model.jacobian_device(eng, U, out=(G, DG))
    eng.mh_langevin_start(U, G, DG)
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert accept() == E.ESTATE                            # no propose since the start
    eng.map_set("exp")
    assert run() == E.ESTATE                               # installed, but no fused kind
    model.ensure_installed(eng)
    assert lib.cesx_mh_langevin_propose(h, 1 << 31, ptr(U), None, ptr(P), None) == E.EINVAL
    assert lib.cesx_mh_langevin_propose(h, 0, ptr(U), None, ptr(U), None) == E.EINVAL
    assert lib.cesx_mh_langevin_propose(h, 0, None, None, ptr(P), None) == E.EINVAL
    assert lib.cesx_mh_langevin_propose(h, 0, ptr(U), None, None, None) == E.EINVAL
    assert propose() == E.OK
    assert lib.cesx_mh_langevin_accept(h, 1 << 31, ptr(U), ptr(P), ptr(G), ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(U), ptr(G), ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(P), None, ptr(DG), None, None) == E.EINVAL
    assert lib.cesx_mh_langevin_accept(h, 0, ptr(U), ptr(P), ptr(G), None, None, None) == E.EINVAL
    assert run(n=0) == E.EINVAL and run(stride=0) == E.EINVAL
    assert run(step=2 ** 31 - 2) == E.EINVAL and run(step=1 << 31) == E.EINVAL
    assert lib.cesx_mh_langevin_run_map(h, 0, 3, 1, None, None, None, None, None) == E.EINVAL
    # the random walk's calls stay refused under a Langevin proposal
    assert lib.cesx_mh_run_map(h, 0, 3, 1, ptr(U), None, None, None, None) == E.EINVAL
    assert lib.cesx_mh_propose(h, 0, ptr(U), None, ptr(P), None) == E.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0)
    steps, rate = eng.mh_stats()
    assert steps == 0 and rate == 0.0
    # and the run goes on: the proposal's map and Jacobian, the accept step, a fused launch
    model.jacobian_device(eng, P, out=(G, DG))
    assert accept() == E.OK
    assert eng.mh_stats()[0] == 1
    assert run() == E.OK
    assert eng.mh_stats()[0] == 4
    with pytest.raises(ValueError, match="noise-free"):
        utils.elliptic(flag_noise=True).jacobian_device(eng, U)
    eng.close()
