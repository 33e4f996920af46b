"""model_mh(chains=M, update='hmc', adapt=) for the linear maps on the device (cesx_mh_hmc_lineal_*, kernels_hmclin.hip): L = 1
against the Langevin step bit for bit, one trajectory position by position against fp64 numpy, the chains against numpy and
the host sampler, the invariance of the exact posterior, the sampler's contracts (reproducibility, resume, alternation with
Langevin steps, shards, NaN, summaries, ABI states) and the adaptation phase, its join and what it is for.  Cases and
references: tests/lineal_hmc_cases.py on tests/lineal_langevin_cases.py, tests/hmc_cases.py and tests/adapt_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapt_cases as ac  # noqa: E402
import chain_summary_cases as cs  # noqa: E402
import lineal_hmc_cases as hl  # noqa: E402
import lineal_langevin_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 1e-9
SIZES = (1, 63, 64, 65, 257)       # ragged vectors for V = 2 and V = 4, and past one workgroup of 128 or 256 chains


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def _states(prob, J, dtype, seed=9):
    """J states from the ensemble's law, already rounded to the engine dtype: the U the engine holds."""
    return lc.exact_draws(prob, J, seed).astype(np.dtype(dtype)).astype(np.float64)


def _started(eng_mod, prob, J, dtype, U0=None, S=None, **kw):
    """An engine with the problem, the Langevin proposal, the model's images and the start states scored, and the buffers of
    a trajectory: (eng, model, U, (Q, Q2, GQ))."""
    eng = eng_mod.Engine(prob["p"], prob["n"], J, dtype=dtype, seed=77, **kw)
    eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["Sigma"], prob["mu"])
    eng.mh_set_proposal("hmc", lc.scales(prob) if S is None else S)
    model = hl.model_of(prob)
    model.langevin_device(eng)
    U = eng.to_device(_states(prob, J, dtype) if U0 is None else U0, prob["p"], "U0").clone()
    eng.mh_langevin_lineal_start(U, model.forward_device(eng, U).clone())
    return eng, model, U, (eng.empty(prob["p"]), eng.empty(prob["p"]), eng.empty(prob["n"]))


def _hmc_step(eng, model, k, U, bufs, L, xi=None, logu=None, poison=None, positions=None):
    """One HMC step through the three entry points, the positions ping-ponging between the two buffers.  ``poison(l, GQ)`` may
    edit the map's rows at position l; ``positions`` collects every Q on the host."""
    Q, Q2, GQ = bufs
    eng.mh_hmc_lineal_begin(k, U, xi=xi, out=Q)
    for l in range(1, L + 1):
        if positions is not None:
            positions.append(eng.to_host(Q).astype(np.float64).copy())
        model.forward_device(eng, Q, out=GQ)
        if poison is not None:
            poison(l, GQ)
        if l < L:
            eng.mh_hmc_lineal_leap(Q, GQ, Q2)
            Q, Q2 = Q2, Q
        else:
            eng.mh_hmc_lineal_accept(k, U, Q, GQ, logu=logu)


def _langevin_step(eng, model, k, U, bufs):
    P, _, GP = bufs
    eng.mh_langevin_lineal_propose(k, U, out=P)
    model.forward_device(eng, P, out=GP)
    eng.mh_langevin_lineal_accept(k, U, P, GP)


def _snapshot(eng, U):
    _, _, per = eng.mh_stats(per_chain=True)
    return eng.to_host(U).copy(), eng.mh_phi().copy(), eng.mh_langevin_lineal_g().copy(), per.copy()


# ---- 1. L = 1 is the Langevin step ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-5x3", (False, True))])
def test_one_leapfrog_is_the_langevin_step_bit_for_bit(eng_mod, name, forms, dtype):
    """Two engines, device noise, 7 steps: cesx_mh_hmc_lineal_begin / _accept against cesx_mh_langevin_lineal_propose / _accept;
    U, phi, g and the per-chain counters are equal."""
    prob = lc.problem(name, *forms)
    for J in (65, 257):
        a, ma, Ua, ba = _started(eng_mod, prob, J, dtype)
        b, mb, Ub, bb = _started(eng_mod, prob, J, dtype)
        for k in range(7):
            _hmc_step(a, ma, k, Ua, ba, 1)
            _langevin_step(b, mb, k, Ub, bb)
        sa, sb = _snapshot(a, Ua), _snapshot(b, Ub)
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y), (name, J, dtype)
        assert 0 < sa[3].sum() < 7 * J and a.mh_stats()[0] == b.mh_stats()[0] == 7
        a.close()
        b.close()


# ---- 2. one trajectory, position by position -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["lineal-5x3", "lineal-17x33", "lineal-65x64"])
def test_a_trajectory_position_by_position(eng_mod, name, dtype):
    """Injected xi, the four forms of Gamma and Sigma, J in SIZES, L in {2, 3, 8}, each trajectory from the states the engine
    holds: on an fp64 engine every Q after the begin and after each leap is within 1e-9 (1 + |Q|) of numpy; on an fp32 engine
    the last Q within 1e-4 (1 + |Q|).  p and n where the update picker changes path.  The lineal maps only: from ensemble draws
    a lineal_log trajectory of 8 leapfrogs overflows exp in the fp64 reference itself for some chains (the chain tests cover
    that map against numpy, where such a trajectory rejects)."""
    worst = 0.0
    for forms in lc.FORMS:
        prob = lc.problem(name, *forms)
        S, p = lc.scales(prob), prob["p"]
        for J in SIZES:
            eng, model, U, bufs = _started(eng_mod, prob, J, dtype)
            rng = np.random.default_rng(100 + J)
            for k, L in enumerate((2, 3, 8)):
                xi = rng.standard_normal((p, J)).astype(np.dtype(dtype)).astype(np.float64)
                Uh = eng.to_host(U).astype(np.float64)
                want = hl.np_positions(prob, S, Uh, xi, L)
                assert np.all(np.isfinite(want[-1]))
                got = []
                _hmc_step(eng, model, k, U, bufs, L, xi=eng.to_device(xi, p, "xi"), positions=got)
                assert len(got) == L
                if dtype == "float64":
                    for q, w in zip(got, want):
                        err = np.abs(q - w) / (1 + np.abs(w))
                        worst = max(worst, float(err.max()))
                        assert np.all(err <= CAP), (name, forms, J, L, float(err.max()))
                else:
                    err = np.abs(got[-1] - want[-1]) / (1 + np.abs(want[-1]))
                    worst = max(worst, float(err.max()))
                    assert np.all(err <= 1e-4), (name, forms, J, L, float(err.max()))
            assert eng.mh_stats()[0] == 3
            eng.close()
    print("\n[lineal hmc] positions %s %s: worst err / (1 + |Q|) %.3g" % (name, dtype, worst))


# ---- 3. the chains against numpy -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-17x33", (False, False))])
def test_1025_chains_against_numpy(eng_mod, name, forms, L, dtype):
    """12 steps of 1 025 chains through MCMC.model_mh with injected noise against ``_hmc_steps``.  fp64: at least 0.999 of the
    chains within 1e-9 (1 + |U|), accept within 1e-12; fp32: at least 0.97 within 1e-4, accept within 0.01 (the caps of
    test_gpu_lineal_langevin.py)."""
    prob = lc.problem(name, *forms)
    M, steps = 1025, 12
    s, enka, prior = hl.sampler(prob, noise="numpy", dtype=dtype, stride=steps)
    np.random.seed(5)
    s.model_mh(hl.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], chains=M, update="hmc", leapfrog=L)
    assert s.fused_launches == 0
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    Ur, acc = hl.np_chains(prob, lc.scales(prob), U0, steps, L, 5)
    rate = acc.sum() / (steps * M)
    Ud = s.samples[:, -1, :]
    tol = 1e-9 if dtype == "float64" else 1e-4
    agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
    print("\n[lineal hmc] %s L=%d %s: agree %.5f accept device %.6f numpy %.6f" % (name, L, dtype, agree.mean(), s.accept, rate))
    assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
    assert abs(s.accept - rate) <= (1e-12 if dtype == "float64" else 0.01)
    assert 0.05 < s.accept < 0.999


# ---- 4. chains=1 is the host sampler -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("adapt", [None, 8])
@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-17x33", (False, False))])
def test_one_chain_equals_the_host_sampler(eng_mod, name, forms, adapt):
    """chains=1 on an fp64 engine under one seed, L = 3, with and without ``adapt=8``: the host sampler's states within
    1e-9 (1 + |U|), its accept rate within 1e-12, and its ``self.adapt``."""
    prob = lc.problem(name, *forms)
    steps, runs = 20, []
    kw = {} if adapt is None else dict(adapt=adapt)
    for chains in (dict(chains=1), {}):
        s, enka, prior = hl.sampler(prob, noise="numpy")
        np.random.seed(13)
        s.model_mh(hl.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], update="hmc", leapfrog=3, **kw, **chains)
        runs.append(s)
    dev, host = runs
    close = lambda x, y: bool(np.all(np.abs(np.asarray(x) - np.asarray(y)) <= CAP * (1 + np.abs(np.asarray(y)))))      # noqa: E731
    assert dev.samples.shape == host.samples.shape == (prob["p"], steps + 1)
    assert close(dev.samples, host.samples)
    assert abs(dev.accept - host.accept) <= 1e-12 and 0 < host.accept <= 1
    if adapt:
        for k in ("multiplier", "delta", "accept_history", "multiplier_history"):
            assert close(dev.adapt[k], host.adapt[k]), k
        assert dev.adapt["steps"] == host.adapt["steps"] == adapt and dev.adapt["multiplier"] != 1.0


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------------------------

def test_gaussian_posterior_is_invariant_on_the_device(eng_mod):
    """16 384 chains from exact posterior draws, lineal-5x3, L = 4, 100 steps with device noise, fp64: the z of the mean and of
    the variances of the final states against m and diag C stay within 5."""
    prob = lc.problem("lineal-5x3", False, False)
    M, steps = 16384, 100
    s, enka, prior = hl.sampler(prob, noise="device", stride=steps)
    enka.Ustar = lc.exact_draws(prob, M, 11)
    s.model_mh(hl.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], chains=M, start="ensemble", update="hmc",
               leapfrog=4)
    zm, zv = lc.moment_z(s.samples[:, -1, :], prob["m"], np.diag(prob["C"]))
    print("\n[lineal hmc] invariance on the device: accept %.4f z mean %s z var %s" % (s.accept, zm, zv))
    assert np.all(zm <= 5) and np.all(zv <= 5), (zm, zv)
    assert 0.05 < s.accept < 0.999


# ---- 6. determinism, resume, alternation -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-5x3", (False, True))])
def test_device_noise_bit_identical_and_exact_resume(eng_mod, name, forms):
    """257 chains, device noise, L = 3: two runs of 12 steps are equal, and 5 + 7 resumed steps end where 12 end."""
    prob = lc.problem(name, *forms)

    def run(splits):
        s, enka, prior = hl.sampler(prob, noise="device", seed=99)
        enka.Ustar = lc.exact_draws(prob, 257, 4)
        for n in splits:
            s.model_mh(hl.model_of(prob), n, prior, enka, prob["Gamma"], delta=prob["delta"], chains=257, start="ensemble",
                       update="hmc", leapfrog=3)
            assert s.fused_launches == 0
        return s.samples
    one = run([12])
    assert np.array_equal(one, run([12]))
    two = run([5, 7])
    assert np.array_equal(one[:, -1, :], two[:, -1, :])
    assert not np.array_equal(one[:, 0, :], one[:, -1, :])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_hmc_and_langevin_steps_alternate_on_one_handle(eng_mod, dtype):
    """257 chains, device noise, the sequence H3 Lv H2 Lv H1 H8 Lv H3 on one handle against the same sequence in which every
    step runs on a FRESH handle started at the states the last one left (cesx_mh_langevin_lineal_start scores phi and g anew):
    U, phi and g after every step and the summed counters are equal bit for bit -- neither family leaves state behind that the
    other reads, and the accept kernels' phi and g are the start's."""
    prob = lc.problem("lineal-17x33", True, True)
    J, seq = 257, (3, 0, 2, 0, 1, 8, 0, 3)
    a, ma, Ua, ba = _started(eng_mod, prob, J, dtype)
    Uh, total = a.to_host(Ua).astype(np.float64), np.zeros(J, dtype=np.int64)
    for k, L in enumerate(seq):
        b, mb, Ub, bb = _started(eng_mod, prob, J, dtype, U0=Uh)
        for eng, m, U, bufs in ((a, ma, Ua, ba), (b, mb, Ub, bb)):
            if L:
                _hmc_step(eng, m, k, U, bufs, L)
            else:
                _langevin_step(eng, m, k, U, bufs)
        sa, sb = _snapshot(a, Ua), _snapshot(b, Ub)
        for x, y in zip(sa[:3], sb[:3]):
            assert np.array_equal(x, y), (k, L)
        total += sb[3].astype(np.int64)
        Uh = sb[0].astype(np.float64)
        b.close()
    assert np.array_equal(total, sa[3].astype(np.int64)) and 0 < total.sum() < len(seq) * J
    a.close()


# ---- 7. shards ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_shard_reproduces_its_global_columns(eng_mod, dtype):
    """An engine over the columns [33, 98) of J_global = 130 reproduces those columns of the whole-range run bit for bit: U,
    counters, phi and g, after 7 steps of L = 3 with device noise."""
    prob = lc.problem("lineal-17x33", True, True)
    lo, hi, Jg = 33, 98, 130
    U0 = _states(prob, Jg, dtype)
    res = []
    for J, off, cols in ((Jg, 0, slice(None)), (hi - lo, lo, slice(lo, hi))):
        eng, model, U, bufs = _started(eng_mod, prob, J, dtype, U0=np.ascontiguousarray(U0[:, cols]), J_global=Jg, j_offset=off)
        for k in range(7):
            _hmc_step(eng, model, k, U, bufs, 3)
        res.append(_snapshot(eng, U))
        eng.close()
    (uw, pw, gw, cw), (us, ps, gs, cs_) = res
    assert np.array_equal(us, uw[:, lo:hi]) and np.array_equal(cs_, cw[lo:hi])
    assert np.array_equal(ps, pw[lo:hi]) and np.array_equal(gs, gw[:, lo:hi]) and 0 < cw.sum() < 7 * Jg


# ---- 8. NaN in mid-trajectory ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("forms", [(False, False), (True, True)], ids=["diagonal", "dense"])
def test_a_nan_in_mid_trajectory_rejects_that_chain_alone(eng_mod, forms, dtype):
    """J = 130, L = 3: a NaN in one row of the map's rows of chain 67 at the second leapfrog.  That chain keeps U, phi and g
    and its counter is 0; every other chain is finite and some, not all, moved."""
    prob = lc.problem("lineal-17x33", *forms)
    J, bad = 130, 67
    eng, model, U, bufs = _started(eng_mod, prob, J, dtype)
    U0, phi0, g0, _ = _snapshot(eng, U)

    def poison(l, GQ):
        if l == 2:
            GQ[5, bad] = float("nan")
    _hmc_step(eng, model, 0, U, bufs, 3, poison=poison)
    U1, phi1, g1, per = _snapshot(eng, U)
    assert per[bad] == 0 and np.array_equal(U1[:, bad], U0[:, bad]) and phi1[bad] == phi0[bad] and np.array_equal(g1[:, bad], g0[:, bad])
    took = per.astype(bool)
    assert 0 < took.sum() < J and np.all(np.isfinite(U1)) and np.all(np.isfinite(g1)) and np.all(np.isfinite(phi1))
    assert np.array_equal(U1[:, ~took], U0[:, ~took]) and np.array_equal(g1[:, ~took], g0[:, ~took])
    assert not np.array_equal(g1[:, took], g0[:, took])
    eng.close()


# ---- 9. adaptation -------------------------------------------------------------------------------------------------------------------------------

def _update_kw(L):
    return dict(update="langevin") if L == 1 else dict(update="hmc", leapfrog=L)


def _target(L):
    return ac.TARGET["langevin" if L == 1 else "hmc"]


@pytest.mark.parametrize("M", [65, 1025])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-5x3", (False, True))])
def test_adaptation_phase_against_numpy(eng_mod, name, forms, L, M):
    """fp64 engine, injected noise, ``adapt=12`` of 13 steps from the ensemble mean at 0.75 x the case's step: the history
    (e_t, abar_t) and the multiplier against ``np_adapt`` within 1e-9, the states after the phase within 1e-9 (1 + |U|)."""
    prob = lc.problem(name, *forms)
    A, f = 12, 0.75
    s, enka, prior = hl.sampler(prob, noise="numpy")
    np.random.seed(5)
    s.model_mh(hl.model_of(prob), A + 1, prior, enka, prob["Gamma"], delta=f * prob["delta"], chains=M, adapt=A, **_update_kw(L))
    S = hl.scales(prob, f)
    U0 = np.repeat(enka.Ustar.mean(axis=1)[:, None], M, axis=1)
    np.random.seed(5)
    states, hist, mult, _ = ac.np_adapt(hl.score_of(prob, S), S, U0, A, L, _target(L))
    ad = s.adapt
    tr = s.samples.reshape(prob["p"], A + 2, M)
    d = ac.differing(tr[:, A, :], states[-1]).sum()
    print("\n[lineal hmc adapt] %s L=%d M=%d: differing %d multiplier %.6f ref %.6f abar_A %.4f" % (name, L, M, d, ad["multiplier"], mult, hist[-1, 1]))
    assert ad["steps"] == A and ad["accept_history"].shape == ad["multiplier_history"].shape == (A,)
    assert np.all(np.abs(ad["multiplier_history"] - hist[:, 0]) <= 1e-9 * (1 + np.abs(hist[:, 0])))
    assert np.all(np.abs(ad["accept_history"] - hist[:, 1]) <= 1e-9)
    assert abs(ad["multiplier"] - mult) <= 1e-9 * mult and d == 0
    assert ad["multiplier_history"][0] == 1.0 and ad["multiplier"] != 1.0 and ad["delta"] == f * prob["delta"] * ad["multiplier"]


def _join_run(prob, adapt, n_mcmc, resume_from=None):
    M = 257
    s, enka, prior = hl.sampler(prob, noise="device", seed=99)
    enka.Ustar = lc.exact_draws(prob, M, 4)
    call = lambda delta, **kw: s.model_mh(hl.model_of(prob), n_mcmc, prior, enka, prob["Gamma"], delta=delta, chains=M,      # noqa: E731
                                          start="ensemble", update="hmc", leapfrog=2, **kw)
    if resume_from is not None:
        s.samples, s._mh_next_step = resume_from.samples[:, :adapt + 1, :].copy(), adapt
        call(resume_from.adapt["delta"])
    else:
        call(0.75 * prob["delta"], adapt=adapt)
    return s


@pytest.mark.parametrize("name, forms", [("lineal-17x33", (True, True)), ("log-5x3", (False, True))])
def test_the_join_is_exact(eng_mod, name, forms):
    """Run X: ``adapt=8`` of 20 steps, device noise, 257 chains.  Run Y: a fresh sampler resumed from X's trace up to step 8 at
    ``delta = X.adapt['delta']`` for 12 steps without ``adapt``: equal states bit for bit, equal ``accept``."""
    prob = lc.problem(name, *forms)
    X = _join_run(prob, 8, 20)
    X2 = _join_run(prob, 8, 20)
    assert np.array_equal(X.samples, X2.samples) and X.accept == X2.accept and X.adapt["multiplier"] == X2.adapt["multiplier"]
    assert X.samples.shape == (prob["p"], 21, 257) and X.fused_launches == 0
    Y = _join_run(prob, 8, 12, resume_from=X)
    assert not hasattr(Y, "adapt")
    assert np.array_equal(Y.samples, X.samples)
    assert X.accept == Y.accept and np.array_equal(X.accept_chains, Y.accept_chains)
    assert 0 < X.accept < 1 and X.adapt["multiplier"] != 1.0


@pytest.mark.parametrize("which", ["long", "short"])
@pytest.mark.parametrize("L", [1, 4])
def test_a_wrong_step_ends_near_the_target(eng_mod, L, which):
    """lineal-17x33 (dense Gamma, dense Sigma), 1 024 chains from the ensemble mean, device noise, delta 8 x too long and 16 x
    too short, ``adapt=100``, then 40 steps: ``accept`` within 0.03 of the target (the numpy reference: within 0.011; the margin
    covers the standard error of 40 x 1 024 tests and a second seed)."""
    prob = lc.problem("lineal-17x33", True, True)
    M = 1024
    s, enka, prior = hl.sampler(prob, noise="device", seed=17, stride=20)
    s.model_mh(hl.model_of(prob), 140, prior, enka, prob["Gamma"], delta=hl.FACTORS[which] * prob["delta"], chains=M, adapt=100,
               **_update_kw(L))
    print("\n[lineal hmc adapt] L=%d %s: multiplier %.4f accept %.4f target %.3f" % (L, which, s.adapt["multiplier"], s.accept, _target(L)))
    assert abs(s.accept - _target(L)) <= 0.03, (s.accept, _target(L))
    assert s.adapt["multiplier"] < 0.5 if which == "long" else s.adapt["multiplier"] > 4.0


def test_a_poisoned_trajectory_has_alpha_zero_and_rejects_alone(eng_mod):
    """65 chains, L = 3, A = 4, injected noise, armed behind the start.  In step 2 chain 7's column of the map's rows is NaN at
    the second leapfrog (a leap), in step 3 chain 40's at the last (the accept): that chain's alpha is 0 and it alone stays;
    the other chains, abar_t and the multiplier match the reference, whose g of that chain is NaN at that position."""
    import torch
    prob = lc.problem("lineal-17x33", True, True)
    J, L, A, p = 65, 3, 4, prob["p"]
    hits = {(2, 2): 7, (3, 3): 40}
    S = hl.scales(prob, 0.75)
    eng, model, U, bufs = _started(eng_mod, prob, J, "float64", S=S)
    U0 = eng.to_host(U).copy()
    eng.mh_adapt_set(A, 0.651)
    np.random.seed(13)
    draws = [(np.random.normal(0, 1, [p, J]), np.log(np.random.uniform(size=J))) for _ in range(A)]
    kept = []
    for t in range(1, A + 1):
        xi, logu = draws[t - 1]

        def poison(l, GQ, t=t):
            if (t, l) in hits:
                GQ[:, hits[(t, l)]] = float("nan")
        _hmc_step(eng, model, t - 1, U, bufs, L, xi=eng.to_device(xi, p, "xi"),
                  logu=torch.as_tensor(logu, dtype=torch.float64, device=eng.device), poison=poison)
        kept.append(eng.to_host(U).copy())
    got = eng.mh_adapt_read()
    eng.close()

    def np_poison(t, l, phq, gq):
        if (t, l) in hits:
            phq[hits[(t, l)]] = np.nan
            gq[:, hits[(t, l)]] = np.nan
    np.random.seed(13)
    states, hist, mult, alphas = ac.np_adapt(hl.score_of(prob, S), S, U0, A, L, 0.651, poison=np_poison)
    assert alphas[1, 7] == 0.0 and alphas[2, 40] == 0.0
    assert np.array_equal(kept[1][:, 7], kept[0][:, 7]) and np.array_equal(kept[2][:, 40], kept[1][:, 40])
    for t in range(A):
        assert not np.any(ac.differing(kept[t], states[t])), t
    assert got["steps"] == A and got["history"].shape == (A, 2)
    assert np.all(np.abs(got["history"] - hist) <= 1e-9 * (1 + np.abs(hist))), got["history"] - hist
    assert abs(got["multiplier"] - mult) <= 1e-9 * mult and np.all(np.isfinite(got["history"]))
    assert 0 < np.sum([not np.array_equal(kept[t], kept[t - 1]) for t in range(1, A)])      # (chains did move)


# ---- 10. ABI states --------------------------------------------------------------------------------------------------------------------------------

def test_abi_states_leave_the_chains_untouched(eng_mod):
    """Every ESTATE / EINVAL case of cesx_mh_hmc_lineal_* returns its code, launches nothing and leaves U and cesx_mh_phi as they
    were; the run then goes on; a cesx_mh_langevin_lineal_propose behind a begin orphans the trajectory; an armed handle runs
    its steps and then refuses."""
    import torch
    E = eng_mod
    prob = lc.problem("lineal-5x3", False, True)
    p, n, M = prob["p"], prob["n"], 30
    S = lc.scales(prob)
    model = hl.model_of(prob)
    eng = E.Engine(p, n, M, dtype="float64")
    lib, h = eng.lib, eng._h
    U = eng.to_device(_states(prob, M, "float64"), p, "U").clone()
    Q, Q2, G = eng.empty(p), eng.empty(p), eng.empty(n)
    DG = torch.as_tensor(np.ascontiguousarray(np.repeat(prob["A"][:, :, None], M, axis=2)), device=eng.device)
    ptr = lambda t: t.data_ptr()      # noqa: E731
    begin = lambda k=0, u=U, q=Q: lib.cesx_mh_hmc_lineal_begin(h, k, None if u is None else ptr(u), None, None if q is None else ptr(q), None)      # noqa: E731
    leap = lambda q=Q, g=G, qn=Q2: lib.cesx_mh_hmc_lineal_leap(h, *(None if t is None else ptr(t) for t in (q, g, qn)), None)      # noqa: E731
    accept = lambda k=0, u=U, q=Q, g=G: lib.cesx_mh_hmc_lineal_accept(h, k, *(None if t is None else ptr(t) for t in (u, q, g)), None, None)      # noqa: E731
    every = lambda: (begin(), leap(), accept())      # noqa: E731

    # no problem, no proposal, a random-walk proposal, no image, no lineal start
    assert every() == (E.ESTATE,) * 3
    eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["Sigma"], prob["mu"])
    assert every() == (E.ESTATE,) * 3
    eng.mh_set_proposal(None, S)
    assert every() == (E.ESTATE,) * 3
    eng.mh_set_proposal("hmc", S)
    assert every() == (E.ESTATE,) * 3                      # no image
    model.langevin_device(eng)
    assert every() == (E.ESTATE,) * 3                      # no start
    model.forward_device(eng, U, out=G)
    eng.mh_langevin_start(U, G, DG)      # the generic start is not the lineal one
    assert every() == (E.ESTATE,) * 3
    eng.mh_langevin_lineal_start(U, G)
    torch.cuda.synchronize()
    U0, phi0 = eng.to_host(U).copy(), eng.mh_phi().copy()
    # the narrow family stays refused behind a lineal start
    assert lib.cesx_mh_hmc_begin(h, 0, ptr(U), None, ptr(Q), None) == E.ESTATE
    assert leap() == E.ESTATE and accept() == E.ESTATE     # no begin
    assert begin(k=1 << 31) == E.EINVAL and begin(q=U) == E.EINVAL and begin(u=None) == E.EINVAL and begin(q=None) == E.EINVAL
    assert leap() == E.ESTATE and accept() == E.ESTATE     # (none of those began)
    assert begin() == E.OK
    assert leap(qn=Q) == E.EINVAL and leap(q=None) == E.EINVAL and leap(g=None) == E.EINVAL and leap(qn=None) == E.EINVAL
    assert accept(k=1 << 31) == E.EINVAL and accept(q=U) == E.EINVAL
    assert accept(u=None) == E.EINVAL and accept(q=None) == E.EINVAL and accept(g=None) == E.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U0) and np.array_equal(eng.mh_phi(), phi0) and eng.mh_stats()[0] == 0
    # and the run goes on: L = 2
    model.forward_device(eng, Q, out=G)
    assert leap() == E.OK
    model.forward_device(eng, Q2, out=G)
    assert accept(q=Q2) == E.OK and eng.mh_stats()[0] == 1
    assert leap() == E.ESTATE and accept() == E.ESTATE     # no begin since the last accept
    # a Langevin proposal behind a begin orphans the trajectory, and a begin behind a proposal the proposal
    assert begin(k=1) == E.OK
    assert lib.cesx_mh_langevin_lineal_propose(h, 1, ptr(U), None, ptr(Q), None) == E.OK
    assert leap() == E.ESTATE and accept(k=1) == E.ESTATE
    assert begin(k=1) == E.OK
    assert lib.cesx_mh_langevin_lineal_accept(h, 1, ptr(U), ptr(Q), ptr(G), None, None) == E.ESTATE
    model.forward_device(eng, Q, out=G)
    assert accept(k=1) == E.OK and eng.mh_stats()[0] == 2

    # armed behind the start: A = 2 steps of L = 2, then the three calls refuse until the proposal is set again
    eng.mh_adapt_set(2, 0.651)
    assert lib.cesx_mh_langevin_lineal_propose(h, 2, ptr(U), None, ptr(Q), None) == E.ESTATE
    for k in (2, 3):
        assert begin(k=k) == E.OK
        model.forward_device(eng, Q, out=G)
        assert leap() == E.OK
        model.forward_device(eng, Q2, out=G)
        assert accept(k=k, q=Q2) == E.OK
    torch.cuda.synchronize()
    U1, phi1 = eng.to_host(U).copy(), eng.mh_phi().copy()
    assert begin(k=4) == E.ESTATE and leap() == E.ESTATE and accept(k=4) == E.ESTATE
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(U), U1) and np.array_equal(eng.mh_phi(), phi1) and eng.mh_stats()[0] == 4
    got = eng.mh_adapt_read()
    assert got["steps"] == 2 and got["history"][0, 0] == 1.0 and np.all((got["history"][:, 1] >= 0) & (got["history"][:, 1] <= 1))
    mult, done = C.c_double(0.0), C.c_int32(0)
    eng.mh_set_proposal("hmc", S)
    assert lib.cesx_mh_adapt_read(h, C.byref(mult), C.byref(done), None) == E.ESTATE
    assert every() == (E.ESTATE,) * 3                      # (the images went with the proposal)
    model.langevin_device(eng)
    model.forward_device(eng, U, out=G)
    eng.mh_langevin_lineal_start(U, G)
    assert begin() == E.OK
    model.forward_device(eng, Q, out=G)
    assert accept() == E.OK and eng.mh_stats()[0] == 1
    # the wrappers check shape, dtype and contiguity
    with pytest.raises(ValueError, match="contiguous"):
        eng.mh_hmc_lineal_begin(0, U[:, :5])
    with pytest.raises(ValueError, match="contiguous"):
        eng.mh_hmc_lineal_leap(Q, G.to(torch.float32), Q2)
    with pytest.raises(ValueError, match="contiguous"):
        eng.mh_hmc_lineal_accept(0, U, Q, G[:, :3])
    eng.close()


# ---- 11. summaries -----------------------------------------------------------------------------------------------------------------------------------

def test_summary_and_marginals_equal_numpy_on_the_trace(eng_mod):
    prob = lc.problem("lineal-5x3", True, False)
    M, steps, p = 257, 24, prob["p"]
    runs = []
    for extra in ({}, dict(summary=True, marginals=True)):
        s, enka, prior = hl.sampler(prob, noise="device", seed=7)
        enka.Ustar = lc.exact_draws(prob, M, 4)
        s.model_mh(hl.model_of(prob), steps, prior, enka, prob["Gamma"], delta=prob["delta"], chains=M, start="ensemble",
                   update="hmc", leapfrog=2, **extra)
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
